"""Table activations end to end on the HIP kernels: golden G21 rebuilt from the reference's bits with the
switches on and off, the nets the lossy-value rule refuses, and model/yolotiny/YoloTiny_fabu.py calibrated on the GPU.  Every
comparison is exact.    pytest -m gpu"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

import activation_nets as an
import depthwise_nets as dn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu
ON = {"concat": True, "shuffle": True, "activations": True}
OFF = {"concat": True, "shuffle": True}


@pytest.fixture(scope="module")
def g21(golden_dir):
    with open(os.path.join(golden_dir, "g21_activation_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g21_activation_net.npz"))


def test_g21_logits_on_the_hip_kernels_with_the_switch_off_on_and_as_a_graph(g21, monkeypatch):
    from common.quantity import _native, resident
    ref, arrays = g21
    want = arrays["logits_recon"]
    x = an.integer_input(an.G21_SHAPE, an.G21_INPUT_SEED).cuda()
    net = dn.rebuild(an.integer_weights(an.g21_net()).eval(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = []
    real = _native.act_lut_i8_nhwc
    monkeypatch.setattr(_native, "act_lut_i8_nhwc", lambda *a, **k: (launches.append(int(a[1])), real(*a, **k))[1])
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries
        off = resident.enable(net, x, **OFF)
        off_logits = net(x).clone()
        np.testing.assert_array_equal(off_logits.cpu().numpy(), want)
        assert "resident_activations" not in off and not launches
        on = resident.enable(net, x, **ON)
        plans = resident.describe(net)
        del launches[:]
        got = net(x)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, off_logits) and launches == [8, 12, 10]
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["resident_activations"] == 3 and not plans.activations_left
        for name in ("conv1", "conv2", "conv3") + an.G21_ACTS:                        # the three producers write no fp32
            assert plans[name].emit_int and not plans[name].emit_f32, (name, plans[name])
        assert on["fp32_outputs"] == 0 and off["fp32_outputs"] == 3
        assert all(plans[a].table.is_cuda for a in an.G21_ACTS)
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


@pytest.mark.parametrize("variant", an.REFUSALS + ("ok",))
def test_the_refusal_nets_give_the_same_logits_with_the_switch_on_and_off(variant):
    from common.quantity import resident
    model = an.RefusalNet(variant).eval().cuda()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        plain = [t.clone() for t in resident._iter_tensors(model(x))]
        resident.enable(model, x, concat=True, avgpool=True)
        off = [t.clone() for t in resident._iter_tensors(model(x))]
        on = resident.enable(model, x, concat=True, avgpool=True, activations=True)
        got = list(resident._iter_tensors(model(x)))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(got, off, plain)) and len(got) == len(off)
    left = resident.describe(model).activations_left
    assert (on["resident_activations"], list(left)) == ((1, []) if variant == "ok" else (0, ["act"])), (on, left)


def _script(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_yolotiny_calibrated_on_the_gpu_keeps_its_logits_and_plans_every_activation():
    """model/yolotiny/YoloTiny_fabu.py, a quarter wide, two heads, 2 images of 64 x 64: calibrated on two batches, rebuilt as the
    integer-simulation model; the resident logits of both heads with and without activations=True are identical, and every one of
    its 19 LeakyReLU modules is a table (the weight seed is one at which the calibration puts the operands of every Concat and
    the readers of every activation on one grid; at others describe() names the few that stay torch's)."""
    from common.quantity import resident
    rf = _script("recon_fuzz")

    def mk():
        return dn.seeded(an.yolo_model(num_outputs=18, width=8, heads=2, batch_norm=False), seed=6).eval().cuda()

    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(2, 3, 64, 64, generator=g).cuda(), torch.zeros(2, dtype=torch.long)) for _ in range(2)]
    out = sys.stdout
    try:
        with product_workdir(input_shape="1,3,64,64", device="gpu", max_cali_img_num=1):
            net = rf.recon_of(mk(), mk(), data)
            x = data[0][0]
            with torch.no_grad():
                plain = [t.clone() for t in net(x)]
                off = resident.enable(net, x, **OFF)
                off_logits = [t.clone() for t in net(x)]
                on = resident.enable(net, x, **ON)
                got = [t.clone() for t in net(x)]
                one = net(x[:1])
            plans = resident.describe(net)
    finally:
        sys.stdout = out
    assert len(got) == 2 and all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(got, off_logits, plain))
    assert all(torch.equal(a, b[:1]) for a, b in zip(one, plain)) and all(float(t.abs().max()) > 0 for t in plain)
    assert plans.activations_left == {} and on["resident_activations"] == 19, (on, plans.activations_left)
    assert on["fp32_outputs"] < off["fp32_outputs"], (on, off)
