"""The small MobileNetV2 of golden G18 end to end on the GPU: the integer-simulation model under
resident.enable(depthwise=True, relu6=True) gives the reference's ReconModel logits bit for bit, plain and captured as a HIP
graph, and a calibration with Quantity.fuse_relu6 writes the tables of one without it and of the reference byte for byte (the
data is integer valued: every engine computes the same tensors).   pytest -m gpu"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import depthwise_nets as dn
import relu6_nets as rn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

BEHIND_RELU6 = ("conv1.0", "blocks.0.dw.0", "blocks.1.expand.0", "blocks.1.dw.0", "blocks.2.expand.0", "blocks.2.dw.0",
                "blocks.3.expand.0", "blocks.3.dw.0", "conv_last.0")


@pytest.fixture(scope="module")
def g18(golden_dir):
    with open(os.path.join(golden_dir, "g18_relu6_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g18_relu6_net.npz"))


def _recon(ref, change=None):
    info = copy.deepcopy(ref["quantity_information"])
    for name, fields in (change or {}).items():
        info[name].update(fields)
    return dn.rebuild(rn.integer_weights(rn.g18_net()).eval(), info).cuda()


def test_reconmodel_with_fused_relu6_gives_the_reference_logits_plain_and_as_a_graph(g18):
    from common.quantity import _native, resident
    ref, arrays = g18
    want = arrays["logits_recon"]
    x = rn.integer_input().cuda()
    net = _recon(ref)
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries, torch's ReLU6
        off = resident.enable(net, x, depthwise=True)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)
        assert "fused_relu6s" not in off and off["fused_relus"] == 0
        on = resident.enable(net, x, depthwise=True, relu6=True)
        plans = resident.describe(net)
        _native.conv_variant_log = {}
        try:
            got = net(x).cpu().numpy()
            log = dict(_native.conv_variant_log)
        finally:
            _native.conv_variant_log = None
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["fused_relu6s"] == len(BEHIND_RELU6) == plans.fused_relu6s and not plans.relu6_left
        assert on["resident_depthwise"] == 4 and on["fp32_outputs"] < off["fp32_outputs"]
        assert all(plans[n].clip and plans[n].relu and plans[n].emit_int for n in BEHIND_RELU6)
        assert not any(plans[n].emit_f32 for n in plans if n.startswith("blocks.")) and not plans["conv1.0"].emit_f32
        assert log.get("depthwise") == 4 and log.get("stem/64") == 1, log              # its own kernels, the stem's included
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


def test_a_layer_forced_off_the_grid_stays_fp32_and_the_logits_stay(g18):
    from common.quantity import resident
    ref, _arrays = g18
    x = rn.integer_input().cuda()
    net = _recon(ref, {"blocks.3.expand.0": {"output_bit": -2, "bias_bit": -2}, "blocks.3.dw.0": {"input_bit": -2}})
    with torch.no_grad():
        plain = net(x)
        on = resident.enable(net, x, depthwise=True, relu6=True)
        plans = resident.describe(net)
        assert on["fused_relu6s"] == len(BEHIND_RELU6) - 1 and list(plans.relu6_left) == ["blocks.3.expand.1"]
        assert plans["blocks.3.expand.0"].emit_f32 and not plans["blocks.3.expand.0"].clip
        assert torch.equal(net(x), plain)


def _calibrate(fuse, trace=None):
    """(feat.table, weight.table as rewritten, timings, the ReLU6 modules a producer served) of one GPU calibration of g18_net."""
    from tools import Quantity
    shape = rn.G18_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="gpu", max_cali_img_num=2) as tmp:
        q = Quantity(rn.integer_weights(rn.g18_net()).eval().cuda())
        q.own_depthwise = True
        if fuse is not None:
            q.fuse_relu6 = fuse
        q.activation_quantize([(x.cuda(), y) for (x, y) in rn.integer_batches(3)])
        wd = os.path.join(tmp, "test", "workdir")
        feat = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        q.rewrite_weight()
        return feat, open(os.path.join(wd, "weight.table")).read(), dict(q.timings), q.fuse_relu6


def test_calibration_with_fused_relu6_writes_the_tables_of_the_reference(g18, monkeypatch):
    from common.quantity import _native
    ref, _arrays = g18
    acts = []
    for name in ("conv1x1_f32", "conv_kxk_f32", "dwconv_f32"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _real=real, _name=name, **k: (acts.append((_name, k.get("act"), k.get("out") is False)),
                                                                                     _real(*a, **k))[1])
    default = _calibrate(None)
    calls_default = list(acts)
    del acts[:]
    off = _calibrate(False)
    calls_off = list(acts)
    del acts[:]
    on = _calibrate(True)
    calls_on = list(acts)
    # off (the default): no call names an activation, the sequence of calls is the default's
    assert calls_off == calls_default and calls_off and all(act is None for (_n, act, _o) in calls_off)
    assert default[:2] == off[:2] and default[3] is False
    # on: the own 1x1 and depthwise convolutions in front of a ReLU6 write the clipped copy, some of them nothing else
    clipped = [c for c in calls_on if c[1] is not None]
    assert clipped and all(act == 6.0 for (_n, act, _o) in clipped) and {n for (n, _a, _o) in clipped} == {"conv1x1_f32", "dwconv_f32"}
    assert on[3] is True                                                   # the once-per-module check against torch's ReLU6 held
    assert on[2]["fused_relus"] == len(BEHIND_RELU6) - 1 and off[2]["fused_relus"] == 0     # (the 3-channel stem runs on the library + the bias producer)
    assert any(alone for (_n, _a, alone) in clipped) or not on[2].get("launches_without_own_output")      # (alone: y not written)
    # the tables: on == off == the reference's, byte for byte
    assert on[0] == off[0] == ref["feat_table"]
    assert on[1] == off[1] == ref["weight_table_rewritten"]
