"""nn.ReLU6 in graph discovery, the tables and the resident integer plan, on a box without a GPU: the exhaustive
integer identity, golden G18 (a small MobileNetV2 through the imported reference, tests/golden/make_golden_relu6.py) on the
oracle-backed engine, and resident.enable(relu6=True) on oracle-backed doubles that follow the reference's fp32 chain literally
(tests/relu6_doubles.py).  Every comparison is exact."""
import copy
import io
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch
from torch import nn

import depthwise_nets as dn
import relu6_doubles as rd
import relu6_nets as rn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_KEYS = {"resident_convs", "resident_adds", "resident_pools", "fused_relus", "fp32_outputs", "int_only_outputs",
               "fused_conv_adds", "fused_block_tails", "fused_projections"}
# the convolutions of relu6_nets.g18_net that an nn.ReLU6 follows directly
BEHIND_RELU6 = ("conv1.0", "blocks.0.dw.0", "blocks.1.expand.0", "blocks.1.dw.0", "blocks.2.expand.0", "blocks.2.dw.0",
                "blocks.3.expand.0", "blocks.3.dw.0", "conv_last.0")


# ---------------------------------------------------------------- 1. the identity and the settings
def test_the_integer_clip_is_relu6_on_every_int8_value_and_output_bit():
    """min(max(q, 0), 6 * 2^ob) * 2^-ob == relu6(q * 2^-ob) in fp32 for every q in [-128, 127] and ob in [-1, 7]; the bound is
    an integer there, is 3 at ob = -1 and the Sp bound 127 from ob = 5 on; below ob = -1 there is no such bound."""
    from common.quantity import _native
    q = torch.arange(-128, 128, dtype=torch.float32)
    for ob in range(-1, 8):
        lo, hi = _native.relu6_clip(ob)
        assert lo == 0 and hi == min(127, int(6 * 2.0 ** ob)) and 6 * 2.0 ** ob == int(6 * 2.0 ** ob)
        scale = torch.tensor(2.0 ** -ob, dtype=torch.float32)
        want = torch.nn.functional.relu6(q * scale)
        got = torch.clamp(q, lo, hi) * scale
        assert torch.equal(got, want), ob
        # ... and Quantity(ob) of the clipped fp32 value is the clipped integer: what the next layer reads
        assert torch.equal(torch.clamp(torch.round(want / scale), -128, 127), torch.clamp(q, lo, hi)), ob
    assert _native.relu6_clip(-1) == (0, 3) and _native.relu6_clip(4) == (0, 96)
    assert all(_native.relu6_clip(ob) == (0, 127) for ob in (5, 6, 7, 12))
    assert all(_native.relu6_clip(ob) is None for ob in (-2, -3, -16))


def test_the_shipped_settings_list_relu6_and_a_call_without_a_clip_is_the_plain_entry_point():
    import yaml
    from common.quantity import _native
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    for key in ("ALL_OP_TYPE", "ALLOW_SAME_TID_OP_TYPE"):
        assert "ReLU6" in settings[key] and "ReLU" in settings[key]
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    lib = _native.lib()
    for name in ("fq_conv2d_i8_resident", "fq_conv2d_i8_resident_pcs", "fq_conv2d_i8_stem", "fq_conv2d_i8_stem_pcs",
                 "fq_dwconv2d_i8_resident", "fq_dwconv2d_i8_resident_pcs", "fq_gconv2d_i8_resident", "fq_gconv2d_i8_resident_pcs"):
        assert re.search(r"^int %s_act\(" % name, text, re.M) and hasattr(lib, name + "_act"), name
        fn, act, what = _native._act_call(name, None, True)                    # no clip: today's call, argument for argument
        assert what == name and act == (1,) and fn is getattr(lib, name)
        assert _native._act_call(name, None, False)[1] == (0,)
        fn, act, what = _native._act_call(name, (0, 96), True)
        assert what == name + "_act" and act == (0, 96) and fn is getattr(lib, name + "_act")
        assert len(getattr(lib, name + "_act").argtypes) == len(getattr(lib, name).argtypes) + 1
        for bad in ((1, 96), (0, 128), (-129, 5), (-5, -1)):
            with pytest.raises(_native.FqError):
                _native._act_call(name, bad, True)
    assert re.search(r"#define\s+FQ_VERSION\s+103\b", text) and lib.fq_version() == 103


def test_the_act_entry_points_check_their_range_before_anything_else():
    """Host arithmetic only (N = 0 launches nothing): a range outside -128 <= lo <= 0 <= hi <= 127 is an invalid argument."""
    from common.quantity import _native
    lib = _native.lib()
    ok = lib.fq_dwconv2d_i8_resident_act(None, None, None, None, 16, 0, 96, 0, 5, 5, 16, 3, 3, 1, 1, 1, 1, 1, 1, 5, 2, None)
    assert ok == 0
    for lo, hi in ((1, 96), (0, 128), (-129, 96), (-4, -1)):
        assert lib.fq_dwconv2d_i8_resident_act(None, None, None, None, 16, lo, hi, 0, 5, 5, 16, 3, 3, 1, 1, 1, 1, 1, 1, 5, 2, None) != 0
        assert lib.fq_gconv2d_i8_resident_act(None, None, None, None, 32, 32, lo, hi, 0, 5, 5, 32, 32, 4, 3, 3, 1, 1, 1, 1, 1, 1, 5, 2,
                                              None) != 0
        assert lib.fq_conv2d_i8_resident_act(None, None, None, None, None, 16, lo, hi, 0, 5, 5, 16, 16, 1, 1, 1, 1, 0, 0, 1, 1, 5, 2,
                                             None) != 0
        assert lib.fq_conv2d_i8_stem_act(None, None, None, None, 16, lo, hi, 0, 3, 8, 8, 16, 3, 3, 2, 2, 1, 1, 4, 5, 2, None) != 0
    assert lib.fq_gconv2d_i8_resident_act(None, None, None, None, 32, 32, 0, 3, 0, 5, 5, 32, 32, 4, 3, 3, 1, 1, 1, 1, 1, 1, 5, 2, None) == 0
    assert lib.fq_conv2d_i8_resident_act(None, None, None, None, None, 16, 0, 3, 0, 5, 5, 16, 16, 1, 1, 1, 1, 0, 0, 1, 1, 5, 2, None) == 0
    assert lib.fq_conv2d_i8_stem_act(None, None, None, None, 16, 0, 3, 0, 3, 8, 8, 16, 3, 3, 2, 2, 1, 1, 4, 5, 2, None) == 0


# ---------------------------------------------------------------- 2. golden G18
@pytest.fixture(scope="module")
def g18(golden_dir):
    with open(os.path.join(golden_dir, "g18_relu6_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g18_relu6_net.npz"))


def _rebuilt(ref, change=None):
    """g18_net as an integer-simulation model from the reference's own bits (ReconModel's module swap, depthwise_nets.rebuild)."""
    info = copy.deepcopy(ref["quantity_information"])
    for name, fields in (change or {}).items():
        info[name].update(fields)
    return dn.rebuild(rn.integer_weights(rn.g18_net()).eval(), info)


def test_g18_data_keeps_the_condition_the_golden_was_made_under(g18):
    ref, _arrays = g18
    ob = {k: v["output_bit"] for k, v in ref["quantity_information"].items()}
    counts = rn.bound_counts(rn.integer_weights(rn.g18_net()).eval(), rn.integer_input())
    assert {k: list(v) for k, v in counts.items()} == ref["bound_counts"] and tuple(counts) == BEHIND_RELU6
    for name in rn.CLIPPED:
        assert ob[name] <= 4 and counts[name][0] > 0 and counts[name][1] > 0
    assert all(ob[name] >= 5 for name in rn.UNCLIPPED) and all(ob[name] >= -1 for name in counts)


def test_g18_cpu_engine_matches_the_reference_and_the_plan_keeps_its_logits(g18, oracle):
    """The reference's graph discovery, merge groups, feat.table and weight.table of the small MobileNetV2 byte for byte through
    the oracle-backed CPU engine on the SHIPPED settings, and its ReconModel logits bit for bit: plain, under the parent's plan,
    with depthwise=True and with depthwise=True, relu6=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g18
    shape = rn.G18_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(rn.integer_weights(rn.g18_net()).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(rn.integer_batches(3))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(rn.integer_weights(rn.g18_net()).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with rd.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = rn.integer_input()
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                for kw in ({}, {"depthwise": True}, {"depthwise": True, "relu6": True}):
                    resident.enable(net, x, **kw)
                    np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"], err_msg=str(kw))
                    np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1], err_msg=str(kw))


# ---------------------------------------------------------------- 3. the plan on the doubles
def test_every_relu6_behind_a_convolution_is_fused_and_nothing_inside_the_blocks_leaves_as_fp32(g18):
    from common.quantity import resident
    ref, arrays = g18
    x = rn.integer_input()
    with rd.installed():
        net = _rebuilt(ref)
        with torch.no_grad():
            plain = net(x)
        np.testing.assert_array_equal(plain.numpy(), arrays["logits_recon"])
        off = resident.enable(net, x, depthwise=True)                     # today: every ReLU6 is foreign code
        off_plans = resident.describe(net)
        assert "fused_relu6s" not in off and off["fused_relus"] == 0 and off_plans.fused_relu6s == 0 and not off_plans.relu6_left
        assert all(off_plans[name].emit_f32 and not off_plans[name].relu for name in BEHIND_RELU6)
        assert not any(p.clip for p in off_plans.values())
        with torch.no_grad():
            assert torch.equal(net(x), plain)
        del rd.calls[:]
        on = resident.enable(net, x, depthwise=True, relu6=True)          # verify=True: bit-identical to the traced forward
        plans = resident.describe(net)
        assert set(on) == PARENT_KEYS | {"resident_depthwise", "fused_relu6s"}
        assert on["fused_relu6s"] == len(BEHIND_RELU6) == plans.fused_relu6s and not plans.relu6_left and on["fused_relus"] == 0
        assert on["resident_depthwise"] == 4 and on["resident_convs"] == off["resident_convs"]
        for name in BEHIND_RELU6:
            p = plans[name]
            assert p.relu and p.clip and p.emit_int and not p.defer, (name, p)
            if name != "conv_last.0":                                     # (the head's pool reads conv_last's exact integers)
                assert not p.emit_f32, (name, p)
        inside = [n for n in plans if n.startswith("blocks.")]
        assert inside and not any(plans[n].emit_f32 for n in inside), {n: plans[n].emit_f32 for n in inside}
        assert not plans["conv1.0"].emit_f32 and on["fp32_outputs"] < off["fp32_outputs"]
        assert not any(p.fuse_next is not None and p.fuse_next.__dict__["_resident"].clip for p in plans.values())
        del rd.calls[:]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        np.testing.assert_array_equal(got.numpy(), arrays["logits_recon"])
        # the bound comes from the layer's output bit at launch; from bit 5 on the launch is the plain fused ReLU's
        ob = {k: v["output_bit"] for k, v in ref["quantity_information"].items()}
        clips = [c for (_n, c) in rd.calls if c is not None]
        want = [(0, 6 << ob[n]) for n in BEHIND_RELU6 if ob[n] < 5]
        assert sorted(clips) == sorted(want * 3) and any(ob[n] >= 5 for n in BEHIND_RELU6)
        # the plan pickles with the model
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert resident.describe(again)["blocks.1.dw.0"].clip and resident.describe(again).fused_relu6s == len(BEHIND_RELU6)
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and resident.describe(net).fused_relu6s == 0
        with torch.no_grad():
            assert torch.equal(net(x), plain)


def test_without_the_argument_the_plan_and_the_calls_are_todays(g18):
    from common.quantity import resident
    ref, _arrays = g18
    x = rn.integer_input()
    fields = [f for f in resident.Plan.__slots__ if f != "fuse_next"]
    with rd.installed():
        net = _rebuilt(ref)
        for kw in ({}, {"depthwise": True}):
            a = resident.enable(net, x, **kw)
            rows_a = {n: tuple(getattr(p, f) for f in fields) for n, p in resident.describe(net).items()}
            del rd.calls[:]
            with torch.no_grad():
                net(x)
            calls_a = list(rd.calls)
            b = resident.enable(net, x, relu6=False, **kw)
            rows_b = {n: tuple(getattr(p, f) for f in fields) for n, p in resident.describe(net).items()}
            del rd.calls[:]
            with torch.no_grad():
                net(x)
            assert a == b and rows_a == rows_b and rows_a and calls_a == rd.calls
            assert "fused_relu6s" not in a and set(a) == PARENT_KEYS | ({"resident_depthwise"} if kw else set())
            assert calls_a and all(clip is None for (_name, clip) in calls_a)      # no launch names a range
            assert not any(isinstance(m.__dict__.get("forward"), resident._ReluPassThrough) for m in net.modules()
                           if isinstance(m, nn.ReLU6))


def test_a_layer_whose_grid_has_no_6_keeps_the_fp32_form_and_describe_says_so(g18):
    from common.quantity import resident
    ref, _arrays = g18
    x = rn.integer_input()
    with rd.installed():
        net = _rebuilt(ref, {"blocks.3.expand.0": {"output_bit": -2, "bias_bit": -2}, "blocks.3.dw.0": {"input_bit": -2}})
        with torch.no_grad():
            plain = net(x)
        on = resident.enable(net, x, depthwise=True, relu6=True)
        plans = resident.describe(net)
        assert on["fused_relu6s"] == len(BEHIND_RELU6) - 1 == plans.fused_relu6s
        assert list(plans.relu6_left) == ["blocks.3.expand.1"] and "output_bit -2" in plans.relu6_left["blocks.3.expand.1"]
        p = plans["blocks.3.expand.0"]
        assert p.emit_f32 and not p.relu and not p.clip                   # today's form: fp32 out, torch's ReLU6, re-quantised
        assert plans["blocks.3.dw.0"].clip and plans["blocks.2.expand.0"].clip
        with torch.no_grad():
            assert torch.equal(net(x), plain)


def test_a_relu6_behind_an_add_stays_torchs():
    """Only a ReLU6 behind a convolution is taken: behind a NewAdd it stays foreign code on the fp32 sum, as without the
    argument, and describe() names it."""
    from common.quantity import resident

    net = dn.SeparableAddNet()
    net.r0, net.r1, net.r2, net.r3 = nn.ReLU6(False), nn.ReLU6(False), nn.ReLU6(False), nn.ReLU(False)
    net = dn.seeded(net.eval())
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    with rd.installed():
        model = dn.rebuild(net, dn.fixed_info(net, out_bits=(3, 4)))
        with torch.no_grad():
            plain = model(x)
        on = resident.enable(model, x, depthwise=True, relu6=True)
        plans = resident.describe(model)
        assert on["fused_relu6s"] == 2 and on["fused_relus"] == 1         # r0 (stem) and r2 (dwb); r3 is an nn.ReLU
        assert list(plans.relu6_left) == ["r1"] and "NewAdd" in plans.relu6_left["r1"]
        assert plans["stem"].clip and plans["dwb"].clip and plans["dwb"].depthwise and not plans["pw"].clip and plans["pw"].relu
        assert plans["Eltwise"].emit_f32 and not plans["Eltwise"].relu
        with torch.no_grad():
            assert torch.equal(model(x), plain)


def test_a_plan_pickled_before_the_slot_existed_still_loads():
    from common.quantity import resident
    p = resident.Plan()
    old = {k: v for k, v in p.__getstate__().items() if k != "clip"}
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(old)
    assert q.clip is False and q.__getstate__() == p.__getstate__()


# ---------------------------------------------------------------- 4. the calibration forward's switch
def test_fuse_relu6_is_off_by_default_and_without_it_no_relu6_module_is_touched():
    """Quantity._patch_fused_convs gives an out-of-place nn.ReLU6 an instance-level forward only with fuse_relu6; without the
    switch the patched set is the parent's (convolutions, the Eltwise, the pool: no activation of this net), and a patched
    ReLU6 whose producer prepared nothing is torch's own module."""
    from tools import Quantity
    from tools._hook_state import _HookState
    assert Quantity.fuse_relu6 is False and Quantity.fuse_relu is True
    with product_workdir(input_shape="1,3,32,32", device="cpu", max_cali_img_num=1):
        q = Quantity(rn.integer_weights(rn.g18_net()).eval())
        q._hook_ctl = _HookState()
        relu6s = [m for m in q.model.modules() if isinstance(m, nn.ReLU6)]
        assert len(relu6s) == len(BEHIND_RELU6)
        off = q._patch_fused_convs(q.model)
        assert off and not any(isinstance(m, nn.ReLU6) for m in off) and not any("forward" in m.__dict__ for m in relu6s)
        for m in off:
            del m.forward
        q.fuse_relu6 = True
        on = q._patch_fused_convs(q.model)
        assert [m for m in on if isinstance(m, nn.ReLU6)] == relu6s and len(on) == len(off) + len(relu6s)
        x = torch.tensor([[-1.0, -0.0, 0.0, 3.5, 6.0, 7.0, float("inf"), float("-inf"), float("nan")]])
        got, want = relu6s[0](x), nn.functional.relu6(x)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        for m in on:
            del m.forward
        inplace = nn.Sequential(nn.Conv2d(3, 4, 1), nn.ReLU6(True))
        assert not any(isinstance(m, nn.ReLU6) for m in q._patch_fused_convs(inplace))        # out-of-place modules only
