"""nn.PixelShuffle / nn.PixelUnshuffle end to end on the HIP kernels: golden G27 rebuilt from the reference's
bits with the switch on, off and as one captured graph, the toy nets of each situation and the nets the plan declines,
model/edsr/EDSR_fabu.py calibrated on the GPU, and eight nets of the random family.  Every comparison is exact.    pytest -m gpu"""
import copy
import io
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import activation_nets as an
import depthwise_nets as dn
import pixelshuffle_nets as pn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu
ALL13 = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
             sums=True, topdown=True, bilinear=True, requant=True, pixelshuffle=True)


@pytest.fixture(scope="module")
def g27(golden_dir):
    with open(os.path.join(golden_dir, "g27_pixelshuffle_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g27_pixelshuffle_net.npz"))


def test_g27_logits_on_the_hip_kernels_with_the_switch_off_on_and_as_a_graph(g27, monkeypatch):
    from common.quantity import _native, resident
    ref, arrays = g27
    want = arrays["logits_recon"]
    x = an.integer_input(pn.G27_SHAPE, pn.G27_INPUT_SEED).cuda()
    net = dn.rebuild(an.integer_weights(pn.g27_net(), base_seed=pn.G27_SEED).eval(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = []
    real = _native.pixel_shuffle_i8_nhwc
    monkeypatch.setattr(_native, "pixel_shuffle_i8_nhwc", lambda x, C, r, inverse, **k: (launches.append((int(C), int(r), int(inverse))),
                                                                                        real(x, C, r, inverse, **k))[1])
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries
        off = resident.enable(net, x)
        off_logits = net(x).clone()
        np.testing.assert_array_equal(off_logits.cpu().numpy(), want)
        assert "resident_pixelshuffles" not in off and not launches
        on = resident.enable(net, x, pixelshuffle=True)
        plans = resident.describe(net)
        del launches[:]
        got = net(x)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, off_logits) and launches == [(8, 2, 1), (8, 2, 0)], (on, plans.pixelshuffle_left)
        assert on["resident_pixelshuffles"] == 1 and on["resident_pixelunshuffles"] == 1 and not plans.pixelshuffle_left
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["fp32_outputs"] == 1 and off["fp32_outputs"] == 3
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.enable(net, x, **ALL13)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


@pytest.mark.parametrize("variant", pn.TOY_VARIANTS)
def test_the_toy_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = pn.ToyNet(variant).eval().cuda()
    x = pn.example().cuda()
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x, **net.kw)
        off = net(x).clone()
        on = resident.enable(net, x, pixelshuffle=True, **net.kw)
        got, one, flipped = net(x).clone(), net(x[:1]).clone(), net(torch.flip(x, dims=[0])).clone()
    assert torch.equal(got, plain) and torch.equal(off, plain) and torch.equal(one, plain[:1])
    assert torch.equal(flipped, torch.flip(plain, dims=[0]))
    plans = resident.describe(net)
    assert on["resident_pixelshuffles"] + on["resident_pixelunshuffles"] == 1 and not plans.pixelshuffle_left
    assert all(plans[n].emit_int and not plans[n].emit_f32 for n in net.fronts)


# ("geometry" needs a predicate patched to refuse and "nd" a Linear on a 3-D input, which the library's fp32 tail does not take --
#  it reads channels at dim 1 --: both run on the CPU doubles only)
@pytest.mark.parametrize("variant", [v for v in sorted(pn.DECLINED) if v not in ("geometry", "nd")] + ["ok"])
def test_the_declined_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = pn.DeclinedNet(variant).eval().cuda()
    x = net.example().cuda()
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x)
        off = net(x).clone()
        on = resident.enable(net, x, pixelshuffle=True)
        got = net(x).clone()
    assert torch.equal(got, off) and torch.equal(got, plain)
    left = resident.describe(net).pixelshuffle_left
    assert (on["resident_pixelshuffles"], list(left)) == ((1, []) if variant == "ok" else (0, ["ps"])), (on, left)
    if variant != "ok":
        assert pn.DECLINED[variant] in left["ps"]


def _script(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _calibrated(mk, shape):
    """(integer-simulation model of the float model mk() calibrated on two random batches, its first batch)"""
    rf = _script("recon_fuzz")
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(*shape, generator=g).cuda(), torch.zeros(shape[0], dtype=torch.long)) for _ in range(2)]
    out = sys.stdout
    try:
        with product_workdir(input_shape="1,3,%d,%d" % shape[2:], device="gpu", max_cali_img_num=1):
            net = rf.recon_of(mk(), mk(), data)
    finally:
        sys.stdout = out
    return net, data[0][0]


@pytest.mark.parametrize("scale", (2, 3))
def test_edsr_calibrated_on_the_gpu_eager_captured_saved_and_disabled(scale, tmp_path):
    """model/edsr/EDSR_fabu.py, two residual blocks of 16 features, 2 images of 16 x 16, calibrated on the GPU (on the parent the
    calibration stops at the tail: the module is unknown to graph discovery).  Outputs bit for bit: eagerly, as a captured graph,
    after a save / load round trip and after disable(); the module is planned and the upsampler's convolution hands on integers
    only."""
    from common.quantity import resident
    net, x = _calibrated(lambda: dn.seeded(pn.edsr_model(scale=scale, n_resblocks=2, n_feats=16), seed=7).eval().cuda(), (2, 3, 16, 16))
    with torch.no_grad():
        plain = net(x).clone()
        off = resident.enable(net, x)
        off_out = net(x).clone()
        on = resident.enable(net, x, pixelshuffle=True)
        plans = resident.describe(net)
        got, one = net(x).clone(), net(x[:1]).clone()
        graphed = resident.capture(net, x)
        replay, replay2 = graphed(x).clone(), graphed(x).clone()
        path = str(tmp_path / "planned.pth")
        torch.save(net, path)
        again = torch.load(path, weights_only=False)
        loaded = again(x).clone()
        resident.disable(net)
        after = net(x).clone()
    print("EDSR x%d 16 x 16: off %s\n on %s\n pixelshuffle_left %s" % (scale, off, on, plans.pixelshuffle_left))
    assert tuple(plain.shape) == (2, 3, 16 * scale, 16 * scale) and float(plain.abs().max()) > 0
    assert torch.equal(got, plain) and torch.equal(off_out, plain) and torch.equal(one, plain[:1])
    assert torch.equal(replay, plain) and torch.equal(replay2, plain) and torch.equal(loaded, plain) and torch.equal(after, plain)
    assert resident.is_enabled(again) and resident.describe(again).keys() == plans.keys() and not resident.describe(net)
    assert on["resident_pixelshuffles"] == 1 and not plans.pixelshuffle_left and "resident_pixelshuffles" not in off
    assert plans["upsampler.1"].up == scale and plans["upsampler.1"].perm == ("d2s", 16)
    assert not plans["upsampler.0"].emit_f32 and on["fp32_outputs"] < off["fp32_outputs"]


def test_eight_random_nets_eagerly_as_one_graph_and_pickled():
    from common.quantity import resident
    planned = 0
    for seed in pn.SEEDS[:8]:
        m = pn.RandomPixelShuffleNet(seed).eval().cuda()
        x = m.example().cuda()
        with torch.no_grad():
            plain = m(x).clone()
            for kw in ({"pixelshuffle": True}, ALL13):
                on = resident.enable(m, x, **kw)
                assert torch.equal(m(x), plain) and torch.equal(m(x[:1]), plain[:1]), (seed, kw)
            graphed = resident.capture(m, x)
            assert torch.equal(graphed(x), plain) and torch.equal(graphed(x), plain), seed
            buf = io.BytesIO()
            pickle.dump(m, buf)
            again = pickle.loads(buf.getvalue())
            assert torch.equal(again(x), plain), seed
        left = resident.describe(m).pixelshuffle_left
        assert on["resident_pixelshuffles"] + on["resident_pixelunshuffles"] + len(left) == len(m.mods_drawn), (seed, on, left)
        planned += on["resident_pixelshuffles"] + on["resident_pixelunshuffles"]
    assert planned >= 8
