"""The re-quantising Concat end to end on the HIP kernels: golden G26 rebuilt from the reference's bits with the
switch on, off and as one captured graph, the toy nets of each cause and the nets the plan declines, and model/unet/UNet_fabu.py and
model/unet/ResUNet_fabu.py calibrated on the GPU.  Every comparison is exact.    pytest -m gpu"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

import activation_nets as an
import depthwise_nets as dn
import bilinear_nets as bn
import requant_nets as rn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu
OFF = {"concat": True, "bilinear": True}
ON = {"concat": True, "bilinear": True, "requant": True}


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.fixture(scope="module")
def g26(golden_dir):
    with open(os.path.join(golden_dir, "g26_requant_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g26_requant_net.npz"))


def test_g26_logits_on_the_hip_kernels_with_the_switch_off_on_and_as_a_graph(g26, monkeypatch):
    from common.quantity import _native, resident
    ref, arrays = g26
    want = arrays["logits_recon"]
    x = an.integer_input(rn.G26_SHAPE, rn.G26_INPUT_SEED).cuda()
    net = dn.rebuild(an.integer_weights(rn.g26_net(), base_seed=rn.G26_SEED).eval(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = []
    real = _native.concat_rq_i8_nhwc
    monkeypatch.setattr(_native, "concat_rq_i8_nhwc",
                        lambda srcs, **k: (launches.append([(int(s[1]), s[0].element_size(), int(s[4])) for s in srcs]), real(srcs, **k))[1])
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries
        off = resident.enable(net, x, **OFF)
        off_logits = net(x).clone()
        np.testing.assert_array_equal(off_logits.cpu().numpy(), want)
        assert "requant_concats" not in off and not launches
        on = resident.enable(net, x, **ON)
        plans = resident.describe(net)
        del launches[:]
        got = net(x)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, off_logits) and len(launches) == on["requant_concats"] >= 1, (on, plans.requant_left)
        assert any(by == 2 for launch in launches for _c, by, _s in launch) and on["requant_sum_sources"] == 1
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["fp32_outputs"] < off["fp32_outputs"]
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


@pytest.mark.parametrize("variant", rn.TOY_VARIANTS)
def test_the_toy_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = rn.ToyNet(variant).eval().cuda()
    x = rn.example().cuda()
    with torch.no_grad():
        plain = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        resident.enable(net, x, concat=True, **net.kw)
        off = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        on = resident.enable(net, x, concat=True, requant=True, **net.kw)
        got = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        one = tuple(t.clone() for t in resident._iter_tensors(net(x[:1])))
        flipped = tuple(t.clone() for t in resident._iter_tensors(net(torch.flip(x, dims=[0]))))
    assert _same(got, plain) and _same(off, plain) and _same(one, tuple(p[:1] for p in plain))
    assert _same(flipped, tuple(torch.flip(p, dims=[0]) for p in plain))
    assert on["requant_concats"] == 1 and not resident.describe(net).requant_left
    assert on["requant_sum_sources"] == (1 if variant in ("sum", "sum_relu") else 0)


@pytest.mark.parametrize("variant", list(rn.DECLINED) + ["ok"])
def test_the_declined_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = rn.DeclinedNet(variant).eval().cuda()
    x = rn.example(2, 8).cuda()
    with torch.no_grad():
        plain = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        resident.enable(net, x, concat=True)
        off = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        on = resident.enable(net, x, concat=True, requant=True)
        got = tuple(resident._iter_tensors(net(x)))
    assert _same(got, off) and _same(got, plain)
    left = resident.describe(net).requant_left
    assert (on["requant_concats"], list(left)) == ((1, []) if variant == "ok" else (0, ["cat"])), (on, left)


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


def test_unet_calibrated_on_the_gpu_plans_every_level_or_says_why():
    """model/unet/UNet_fabu.py, base width 8, depth 2, 4 images of 32 x 32, calibrated on the GPU: with requant=True the outputs
    are the plain forward's bit for bit, eagerly and as a captured graph, and every bilinear upsampling and every Concat is planned
    or named with its reason."""
    from common.quantity import resident
    net, x = _calibrated(lambda: dn.seeded(bn.unet_model(num_classes=3, input_size=32, base_width=8, depth=2, batch_norm=False), seed=6).eval().cuda(),
                         (4, 3, 32, 32))
    with torch.no_grad():
        plain = net(x).clone()
        off = resident.enable(net, x, **OFF)
        off_out = net(x).clone()
        on = resident.enable(net, x, **ON)
        got, one = net(x).clone(), net(x[:1]).clone()
        graphed = resident.capture(net, x)
        replay, replay2 = graphed(x).clone(), graphed(x).clone()
    plans = resident.describe(net)
    print("UNet 32 x 32: off %s\n on %s\n bilinear_left %s requant_left %s" % (off, on, plans.bilinear_left, plans.requant_left))
    assert torch.equal(got, plain) and torch.equal(off_out, plain) and torch.equal(one, plain[:1])
    assert torch.equal(replay, plain) and torch.equal(replay2, plain)
    assert on["resident_bilinears"] + len(plans.bilinear_left) == 2 and on["resident_bilinears"] >= off["resident_bilinears"]
    assert on["fp32_outputs"] <= off["fp32_outputs"]


def test_resunet_calibrated_on_the_gpu_eager_captured_saved_and_disabled(tmp_path):
    """model/unet/ResUNet_fabu.py, base width 8, one block per stage, 2 images of 64 x 64, calibrated on the GPU: every Concat
    joins the int16 sum of a stage with a bilinear upsampling.  Outputs bit for bit: eagerly, as a captured graph, after a save /
    load round trip and after disable(); the counts are printed, and each Concat is planned or named with its reason."""
    from common.quantity import resident
    net, x = _calibrated(lambda: dn.seeded(rn.resunet_model(num_classes=3, input_size=64, base_width=8, layers=(1, 1, 1, 1), batch_norm=False),
                                           seed=7).eval().cuda(), (2, 3, 64, 64))
    with torch.no_grad():
        plain = net(x).clone()
        off = resident.enable(net, x, **OFF)
        off_out = net(x).clone()
        on = resident.enable(net, x, **ON)
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
    print("ResUNet 64 x 64: off %s\n on %s\n bilinear_left %s requant_left %s" % (off, on, plans.bilinear_left, plans.requant_left))
    assert tuple(plain.shape) == (2, 3, 16, 16) and float(plain.abs().max()) > 0
    assert torch.equal(got, plain) and torch.equal(off_out, plain) and torch.equal(one, plain[:1])
    assert torch.equal(replay, plain) and torch.equal(replay2, plain) and torch.equal(loaded, plain) and torch.equal(after, plain)
    assert resident.is_enabled(again) and resident.describe(again).keys() == plans.keys() and not resident.describe(net)
    assert on["requant_concats"] + len(plans.requant_left) == 3 and "requant_concats" not in off
    assert on["requant_sum_sources"] == on["requant_concats"] and on["fp32_outputs"] <= off["fp32_outputs"]
