"""Bilinear upsampling end to end on the HIP kernels: golden G25 rebuilt from the reference's bits with the
switch on and off, the two-level decoder nets and the nets the plan declines, and model/unet/UNet_fabu.py calibrated on the GPU,
run eagerly and as a captured graph.  Every comparison is exact.    pytest -m gpu"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

import activation_nets as an
import bilinear_nets as bn
import depthwise_nets as dn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu
ON = {"concat": True, "bilinear": True}
OFF = {"concat": True}


@pytest.fixture(scope="module")
def g25(golden_dir):
    with open(os.path.join(golden_dir, "g25_bilinear_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g25_bilinear_net.npz"))


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def test_g25_logits_on_the_hip_kernels_with_the_switch_off_on_and_as_a_graph(g25, monkeypatch):
    from common.quantity import _native, resident
    ref, arrays = g25
    want = arrays["logits_recon"]
    x = an.integer_input(bn.G25_SHAPE, bn.G25_INPUT_SEED).cuda()
    net = dn.rebuild(an.integer_weights(bn.g25_net(), base_seed=bn.G25_SEED).eval(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = []
    real = _native.upsample_bilinear_i8_nhwc
    monkeypatch.setattr(_native, "upsample_bilinear_i8_nhwc", lambda *a, **k: (launches.append((int(a[1]), int(a[2]), bool(a[4]))), real(*a, **k))[1])
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries
        off = resident.enable(net, x, **OFF)
        off_logits = net(x).clone()
        np.testing.assert_array_equal(off_logits.cpu().numpy(), want)
        assert "resident_bilinears" not in off and not launches
        on = resident.enable(net, x, **ON)
        plans = resident.describe(net)
        del launches[:]
        got = net(x)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, off_logits) and launches == [(12, 2, True), (8, 2, False), (8, 4, False)]
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["resident_bilinears"] == 3 and not plans.bilinear_left and on["resident_concats"] == 2
        for name in ("conv4", "conv5", "conv7") + bn.G25_UPS:                          # the three producers write no fp32
            assert plans[name].emit_int and not plans[name].emit_f32, (name, plans[name])
        assert on["fp32_outputs"] < off["fp32_outputs"]
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


@pytest.mark.parametrize("variant", bn.DECODER_VARIANTS)
def test_the_decoder_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = bn.DecoderNet(variant).eval().cuda()
    x = bn.example().cuda()
    with torch.no_grad():
        plain = net(x).clone()
        resident.enable(net, x, concat=True, shuffle=True)
        off = net(x).clone()
        on = resident.enable(net, x, concat=True, shuffle=True, bilinear=True)
        assert torch.equal(net(x), plain) and torch.equal(off, plain)
        assert torch.equal(net(x[:1]), plain[:1]) and torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
    assert on["resident_bilinears"] == len(net.ups) and not resident.describe(net).bilinear_left
    assert on["fp32_outputs"] == 1


@pytest.mark.parametrize("variant", list(bn.DECLINED) + ["ok"])
def test_the_declined_nets_give_the_same_outputs_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    net = bn.DeclinedNet(variant).eval().cuda()
    x = bn.example(2, 8).cuda()
    kw = dict(concat=True, activations=variant in ("lossy", "act"))
    with torch.no_grad():
        plain = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        resident.enable(net, x, **kw)
        off = tuple(t.clone() for t in resident._iter_tensors(net(x)))
        on = resident.enable(net, x, bilinear=True, **kw)
        got = tuple(resident._iter_tensors(net(x)))
    assert _same(got, off) and _same(got, plain)
    left = resident.describe(net).bilinear_left
    assert (on["resident_bilinears"], list(left)) == ((1, []) if variant == "ok" else (0, ["up"])), (on, left)


def _script(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_unet_calibrated_on_the_gpu_keeps_its_outputs_eagerly_and_as_a_graph():
    """model/unet/UNet_fabu.py, base width 8, depth 2, 4 images of 32 x 32: calibrated on two batches, rebuilt as the
    integer-simulation model; the resident outputs with and without bilinear=True are the plain forward's bit for bit, eagerly
    and as a captured graph.  Every bilinear upsampling is planned or named with its reason (where the calibration puts a Concat's
    reader on another bit than its skip, the lossy verification takes the upsampling back and says so); the count is printed."""
    from common.quantity import resident
    rf = _script("recon_fuzz")

    def mk():
        return dn.seeded(bn.unet_model(num_classes=3, input_size=32, base_width=8, depth=2, batch_norm=False), seed=6).eval().cuda()

    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(4, 3, 32, 32, generator=g).cuda(), torch.zeros(4, dtype=torch.long)) for _ in range(2)]
    out = sys.stdout
    try:
        with product_workdir(input_shape="1,3,32,32", device="gpu", max_cali_img_num=1):
            net = rf.recon_of(mk(), mk(), data)
            x = data[0][0]
            with torch.no_grad():
                plain = net(x).clone()
                off = resident.enable(net, x, **OFF)
                off_out = net(x).clone()
                on = resident.enable(net, x, **ON)
                got = net(x).clone()
                one = net(x[:1]).clone()
                graphed = resident.capture(net, x)
                replay = graphed(x).clone()
                replay2 = graphed(x).clone()
            plans = resident.describe(net)
    finally:
        sys.stdout = out
    print("UNet 32 x 32: off %s\n on %s\n left %s" % (off, on, plans.bilinear_left))
    assert tuple(plain.shape) == (4, 3, 32, 32) and float(plain.abs().max()) > 0
    assert torch.equal(got, plain) and torch.equal(off_out, plain) and torch.equal(one, plain[:1])
    assert torch.equal(replay, plain) and torch.equal(replay2, plain)
    assert on["resident_bilinears"] + len(plans.bilinear_left) == 2 and "resident_bilinears" not in off
    assert on["fp32_outputs"] <= off["fp32_outputs"]
