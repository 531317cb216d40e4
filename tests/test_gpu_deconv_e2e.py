"""nn.ConvTranspose2d end to end on the HIP kernels: golden G28 rebuilt from the reference's bits with the switch
off, on, as one captured graph and with all fourteen switches, the toy nets of each situation and the nets the plan declines,
model/unet/UNet_fabu.py with up="deconv" calibrated on the GPU, and eight nets of the random family.  Every comparison is exact.
pytest -m gpu"""
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
import deconv_nets as dn
import depthwise_nets
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu
ALL14 = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
             sums=True, topdown=True, bilinear=True, requant=True, pixelshuffle=True, deconv=True)


@pytest.fixture(scope="module")
def g28(golden_dir):
    with open(os.path.join(golden_dir, "g28_deconv_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g28_deconv_net.npz"))


def _counting(monkeypatch):
    from common.quantity import _native
    launches = []
    real = _native.deconv2d_i8_resident

    def counted(xq, wq, qbias, C, kernel, *a, **k):
        launches.append((int(C), qbias.numel(), tuple(kernel)))
        return real(xq, wq, qbias, C, kernel, *a, **k)

    monkeypatch.setattr(_native, "deconv2d_i8_resident", counted)
    return launches


def test_g28_twin_logits_on_the_hip_kernels_with_the_switch_off_on_captured_and_all_fourteen(g28, monkeypatch):
    """The net that ends behind conv2, rebuilt from the bits the reference wrote for it and for its twin: the logits of the
    reference's own ReconModel of the twin, bit for bit."""
    from common.quantity import resident
    ref, arrays = g28
    want = arrays["logits_twin_recon"]
    x = an.integer_input(dn.G28_SHAPE, dn.G28_INPUT_SEED).cuda()
    net = dn.rebuild(dn.g28_net(head_only=True), copy.deepcopy(ref["twin"]["head_quantity_information"])).cuda()
    launches = _counting(monkeypatch)
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # the reference-shaped form: torch's module
        net.up1.use_deconv_i8 = True
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # per instance: the kernel, fp32 out
        assert launches == [(8, 8, (2, 2))]
        net.up1.use_deconv_i8 = False
        off = resident.enable(net, x)
        off_logits = net(x).clone()
        np.testing.assert_array_equal(off_logits.cpu().numpy(), want)
        assert "resident_deconvs" not in off and len(launches) == 1
        on = resident.enable(net, x, deconv=True)
        plans = resident.describe(net)
        del launches[:]
        got = net(x)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, off_logits) and launches == [(8, 8, (2, 2))], (on, plans.deconv_left)
        assert on["resident_deconvs"] == 1 and not plans.deconv_left and plans["up1"].relu and not plans["conv1"].emit_f32
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["fp32_outputs"] == 1 and off["fp32_outputs"] == 2
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.enable(net, x, **ALL14)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


def test_g28_full_net_on_the_hip_kernels_with_the_switch_off_on_captured_and_all_fourteen(g28, monkeypatch):
    from common.quantity import resident
    ref, _arrays = g28
    x = an.integer_input(dn.G28_SHAPE, dn.G28_INPUT_SEED).cuda()
    net = dn.rebuild(dn.g28_net(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = _counting(monkeypatch)
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x)
        off = net(x).clone()
        assert not launches
        on = resident.enable(net, x, deconv=True)
        del launches[:]
        got, one = net(x).clone(), net(x[:1]).clone()
        assert launches == [(8, 8, (2, 2)), (8, 4, (4, 4))] * 2
        graphed = resident.capture(net, x)
        replay, replay2 = graphed(x).clone(), graphed(x).clone()
        resident.enable(net, x, **ALL14)
        every = net(x).clone()
    assert tuple(plain.shape) == (4, 3, 64, 64) and float(plain.std()) > 0
    assert torch.equal(got, plain) and torch.equal(off, plain) and torch.equal(one, plain[:1]) and torch.equal(every, plain)
    assert torch.equal(replay, plain) and torch.equal(replay2, plain)
    assert on["resident_deconvs"] == 2 and not resident.describe(net).deconv_left


@pytest.mark.parametrize("variant", dn.TOY_VARIANTS)
def test_the_toy_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = dn.ToyNet(variant).eval().cuda()
    x = dn.example().cuda()
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x, **net.kw)
        off = net(x).clone()
        on = resident.enable(net, x, deconv=True, **net.kw)
        got, one, flipped = net(x).clone(), net(x[:1]).clone(), net(torch.flip(x, dims=[0])).clone()
    assert torch.equal(got, plain) and torch.equal(off, plain) and torch.equal(one, plain[:1])
    assert torch.equal(flipped, torch.flip(plain, dims=[0])) and float(plain.abs().max()) > 0
    plans = resident.describe(net)
    assert on["resident_deconvs"] == 1 and not plans.deconv_left
    assert all(plans[n].emit_int and not plans[n].emit_f32 for n in net.fronts)


@pytest.mark.parametrize("variant", sorted(dn.DECLINED) + ["ok"])
def test_the_declined_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = dn.DeclinedNet(variant).eval().cuda()
    x = dn.example().cuda()
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x)
        off = net(x).clone()
        on = resident.enable(net, x, deconv=True)
        got = net(x).clone()
    assert torch.equal(got, off) and torch.equal(got, plain)
    left = resident.describe(net).deconv_left
    assert (on["resident_deconvs"], list(left)) == ((1, []) if variant == "ok" else (0, ["up"])), (on, left)
    if variant != "ok":
        assert dn.DECLINED[variant] in left["up"]


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


@pytest.mark.parametrize("up_kernel", (2, 3, 4))
def test_unet_with_up_convolutions_calibrated_on_the_gpu_eager_captured_saved_and_disabled(up_kernel, tmp_path):
    """model/unet/UNet_fabu.py with up="deconv", base width 8, depth 2, 2 images of 32 x 32, calibrated on the GPU (on the parent the
    calibration stops behind the first up-convolution: the type is unknown to graph discovery).  Outputs bit for bit: eagerly, as a
    captured graph, after a save / load round trip and after disable(); both up-convolutions are planned and the level in front of
    each hands on integers only."""
    from common.quantity import NewConvTranspose2d, resident
    mk = lambda: depthwise_nets.seeded(dn.unet_model(input_size=32, base_width=8, depth=2, batch_norm=False, up="deconv",  # noqa: E731
                                                     up_kernel=up_kernel), seed=7).eval().cuda()
    net, x = _calibrated(mk, (2, 3, 32, 32))
    assert all(isinstance(u, NewConvTranspose2d) for u in net.ups)
    kw = dict(concat=True, requant=True)
    with torch.no_grad():
        plain = net(x).clone()
        off = resident.enable(net, x, **kw)
        off_out = net(x).clone()
        on = resident.enable(net, x, deconv=True, **kw)
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
    print("UNet up_kernel %d 32 x 32: off %s\n on %s\n deconv_left %s" % (up_kernel, off, on, plans.deconv_left))
    assert tuple(plain.shape) == (2, 2, 32, 32) and float(plain.abs().max()) > 0
    assert torch.equal(got, plain) and torch.equal(off_out, plain) and torch.equal(one, plain[:1])
    assert torch.equal(replay, plain) and torch.equal(replay2, plain) and torch.equal(loaded, plain) and torch.equal(after, plain)
    assert resident.is_enabled(again) and resident.describe(again).keys() == plans.keys() and not resident.describe(net)
    assert on["resident_deconvs"] == 2 and not plans.deconv_left and "resident_deconvs" not in off
    assert "ups.0" in plans and "ups.1" in plans and on["fp32_outputs"] < off["fp32_outputs"]
    assert not plans["downs.1.2"].emit_f32 and not plans["decs.0.2"].emit_f32


def test_eight_random_nets_eagerly_as_one_graph_and_pickled():
    from common.quantity import resident
    planned = 0
    for seed in dn.SEEDS[:8]:
        m = dn.RandomDeconvNet(seed).eval().cuda()
        x = m.example().cuda()
        with torch.no_grad():
            plain = m(x).clone()
            for kw in ({"deconv": True}, ALL14):
                on = resident.enable(m, x, **kw)
                assert torch.equal(m(x), plain) and torch.equal(m(x[:1]), plain[:1]), (seed, kw)
            graphed = resident.capture(m, x)
            assert torch.equal(graphed(x), plain) and torch.equal(graphed(x), plain), seed
            buf = io.BytesIO()
            pickle.dump(m, buf)
            again = pickle.loads(buf.getvalue())
            assert torch.equal(again(x), plain), seed
        left = resident.describe(m).deconv_left
        assert on["resident_deconvs"] + len(left) == len(m.ups), (seed, on, left)
        planned += on["resident_deconvs"]
    assert planned >= 8
