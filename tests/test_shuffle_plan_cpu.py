"""nn.ChannelShuffle and the Slice marker in graph discovery, the tables and the resident integer plan, on a box without a GPU
(DESIGN section 23): golden G20 (a toy ShuffleNetV2 through the imported reference, tests/golden/make_golden_shuffle.py) on the
oracle-backed engine, resident.enable(shuffle=True) on oracle-backed doubles (tests/shuffle_doubles.py: the index rule in numpy,
held against the reference's fp32 chain), what the plan leaves in fp32 form and why, the host arithmetic of fq_shuffle_i8_nhwc,
and the kernel's address arithmetic walked on the host (scripts/shuffle_geom_check.cpp).  Every comparison is exact."""
import copy
import ctypes
import io
import json
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import depthwise_nets as dn
import shuffle_doubles as sd
import shuffle_nets as sn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, UNSUPPORTED = -1, -4
UNIT_CONVS = tuple("units.%d.%s" % (k, n) for k in range(3) for n in ("branch.0.0", "branch.1.0", "branch.2.0")) \
    + ("units.0.down.0.0", "units.0.down.1.0")
# resident.enable on the G20 net at the PARENT commit (cf63a02), recorded by running that commit on the same doubles: the summary
# per set of switches, and (emit_f32, emit_int, relu) of every planned module under depthwise=True, concat=True
PARENT = {
    (): {"resident_convs": 9, "resident_adds": 0, "resident_pools": 2, "fused_relus": 9, "fp32_outputs": 8, "int_only_outputs": 2,
         "fused_conv_adds": 0, "fused_block_tails": 0, "fused_projections": 0},
    ("depthwise",): {"resident_convs": 13, "resident_adds": 0, "resident_pools": 2, "fused_relus": 9, "fp32_outputs": 4,
                     "int_only_outputs": 10, "resident_depthwise": 4, "fused_conv_adds": 0, "fused_block_tails": 0,
                     "fused_projections": 0},
    ("depthwise", "concat"): {"resident_convs": 13, "resident_adds": 0, "resident_pools": 2, "fused_relus": 9, "fp32_outputs": 3,
                              "int_only_outputs": 12, "resident_depthwise": 4, "resident_concats": 1, "resident_upsamples": 0,
                              "fused_conv_adds": 0, "fused_block_tails": 0, "fused_projections": 0, "fused_upsamples": 0},
    ("depthwise", "concat", "flatten"): {"resident_convs": 13, "resident_adds": 0, "resident_pools": 2, "fused_relus": 9,
                                         "fp32_outputs": 3, "int_only_outputs": 12, "resident_depthwise": 4, "resident_concats": 1,
                                         "resident_upsamples": 0, "flattened_concats": 0, "fused_conv_adds": 0,
                                         "fused_block_tails": 0, "fused_projections": 0, "fused_upsamples": 0},
}
PARENT_ROWS = [("conv1.0", False, True, True), ("conv5.0", False, True, True), ("maxpool", False, True, False),
               ("units.0.Concat", True, False, False), ("units.0.branch.0.0", False, True, True),
               ("units.0.branch.1.0", False, True, False), ("units.0.branch.2.0", False, True, True),
               ("units.0.down.0.0", False, True, False), ("units.0.down.1.0", False, True, True),
               ("units.1.branch.0.0", False, True, True), ("units.1.branch.1.0", False, True, False),
               ("units.1.branch.2.0", True, False, True), ("units.2.branch.0.0", False, True, True),
               ("units.2.branch.1.0", False, True, False), ("units.2.branch.2.0", True, False, True)]
ON = {"depthwise": True, "concat": True, "shuffle": True}


@pytest.fixture(scope="module")
def g20(golden_dir):
    with open(os.path.join(golden_dir, "g20_shuffle_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g20_shuffle_net.npz"))


def _rebuilt(ref):
    """g20_net as an integer-simulation model from the reference's own bits (ReconModel's module swap, depthwise_nets.rebuild)."""
    return dn.rebuild(sn.integer_weights(sn.g20_net()).eval(), copy.deepcopy(ref["quantity_information"]))


# ---------------------------------------------------------------- 1. settings, marker, golden G20
def test_the_shipped_settings_list_the_two_names_and_the_marker_is_exported():
    import yaml
    import common.quantity as cq
    from common.quantity import fabu_layer
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    assert "ChannelShuffle" in settings["ALL_OP_TYPE"] and "ChannelShuffle" in settings["ALLOW_SAME_TID_OP_TYPE"]
    assert "Slice" in settings["ALL_OP_TYPE"] and "Slice" not in settings["ALLOW_SAME_TID_OP_TYPE"]
    assert not {"ChannelShuffle", "Slice"} & (set(settings["CARE_OP_TYPE"]) | set(settings["MERGE_OP_YTPE"]))
    assert cq.Slice is fabu_layer.Slice is sn.Slice and "Slice" in cq.__all__ and "Slice" in fabu_layer.__all__
    x = torch.arange(2 * 6 * 2 * 2, dtype=torch.float32).reshape(2, 6, 2, 2)
    y = cq.Slice(1, 4)(x)
    assert torch.equal(y, x[:, 1:4]) and y.data_ptr() != x[:, 1:4].data_ptr() and y.is_contiguous()      # a fresh tensor
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    assert re.search(r"^int fq_shuffle_i8_nhwc\(", text, re.M) and re.search(r"^int fq_shuffle_i8_nhwc_supported\(", text, re.M)
    from common.quantity import _native
    assert re.search(r"#define\s+FQ_VERSION\s+103\b", text) and _native.lib().fq_version() == 103


def test_g20_merge_groups_chain_the_concats_of_consecutive_units(g20):
    ref, _arrays = g20
    info, groups = ref["net_info"], ref["merge_groups"]
    cats = [n for n in ref["net_info_order"] if info[n]["type"] == "Concat"]
    assert len(cats) == 3 and not any(v["type"] in ("ChannelShuffle", "Slice") for v in info.values())      # pruned one-input ops
    for a, b in zip(cats, cats[1:]):
        assert a in info[b]["inputs"] and any(sorted(g) == sorted(info[b]["inputs"]) for g in groups), (a, b, groups)
    q = ref["quantity_information"]
    grids = set(q[c]["input_bit"] for c in sn.CONCATS) | set(q["units.%d.branch.2.0" % k]["output_bit"] for k in range(3))
    assert len(grids | {q["units.0.down.1.0"]["output_bit"]}) == 1                                       # one grid for every operand
    # the layer behind a slice / shuffle takes the input bit of the cared layer in front
    for k in (1, 2):
        assert q["units.%d.branch.0.0" % k]["input_bit"] == q["units.%d.Concat" % (k - 1)]["output_bit"]
    assert q["conv5.0"]["input_bit"] == q["units.2.Concat"]["output_bit"]


def test_g20_cpu_engine_matches_the_reference_and_the_plan_keeps_its_logits(g20, oracle):
    """The reference's graph discovery, merge groups, feat.table and both weight.tables of the toy ShuffleNetV2 byte for byte
    through the oracle-backed CPU engine on the SHIPPED settings, and its ReconModel logits bit for bit: plain, under the parent's
    switches and with shuffle=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g20
    shape = sn.G20_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(sn.integer_weights(sn.g20_net()).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(sn.integer_batches(3))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(sn.integer_weights(sn.g20_net()).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with sd.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = sn.integer_input()
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                for kw in ({}, {"depthwise": True, "concat": True}, ON):
                    resident.enable(net, x, **kw)
                    np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"], err_msg=str(kw))
                    np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1], err_msg=str(kw))


# ---------------------------------------------------------------- 2. the plan on the doubles
def test_every_shuffle_and_slice_is_planned_and_nothing_between_stem_and_head_leaves_as_fp32(g20):
    from common.quantity import resident
    ref, arrays = g20
    x = sn.integer_input()
    with sd.installed():
        net = _rebuilt(ref)
        with torch.no_grad():
            plain = net(x)
        np.testing.assert_array_equal(plain.numpy(), arrays["logits_recon"])
        off = resident.enable(net, x, depthwise=True, concat=True)
        with torch.no_grad():
            off_logits = net(x)
        assert not sd.calls                                               # without the switch: no launch of the new entry point
        on = resident.enable(net, x, **ON)                               # verify=True: bit-identical to the traced forward
        plans = resident.describe(net)
        assert set(on) == set(off) | {"resident_shuffles", "resident_slices"}
        assert on["resident_shuffles"] == 3 and on["resident_slices"] == 4 and on["resident_concats"] == 3
        assert on["resident_depthwise"] == 4 and on["resident_convs"] == off["resident_convs"] and not plans.shuffle_left
        # every unit conv hands on integers only; so do the markers: nobody in this net needs fp32 before the head's pool
        for name in UNIT_CONVS + sn.SHUFFLES + sn.SLICES + sn.CONCATS + ("conv1.0", "maxpool"):
            p = plans[name]
            assert p.emit_int and not p.emit_f32, (name, p)
        assert on["fp32_outputs"] == 0 and on["int_only_outputs"] == len(plans) == 24 and off["fp32_outputs"] == 3
        assert [plans[n].perm for n in sn.SHUFFLES] == [(0, 20, 2)] * 3
        assert [plans[n].perm for n in sn.SLICES] == [(0, 10, 1), (10, 10, 1)] * 2
        assert not any(plans[n].relu for n in sn.SHUFFLES + sn.SLICES)
        assert all(p.perm is None for n, p in plans.items() if n not in sn.SHUFFLES + sn.SLICES)
        del sd.calls[:]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(got, off_logits) and torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        np.testing.assert_array_equal(got.numpy(), arrays["logits_recon"])
        per_forward = [(20, 0, 20, 2), (20, 0, 10, 1), (20, 10, 10, 1), (20, 0, 20, 2), (20, 0, 10, 1), (20, 10, 10, 1), (20, 0, 20, 2)]
        assert [c[:4] for c in sd.calls] == per_forward * 3 and all(c[4][3] == 32 for c in sd.calls)
        # save, load: the plan pickles with the model; re-enable: the same logits
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert resident.describe(again)["units.1.right"].perm == (10, 10, 1)
        with torch.no_grad():
            assert torch.equal(again(x), plain)
            assert resident.enable(again, x, **ON) == on
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and not resident.describe(net).shuffle_left
        with torch.no_grad():
            assert torch.equal(net(x), plain)


def test_without_the_switch_the_summary_and_the_plan_are_the_parents(g20):
    from common.quantity import resident
    ref, _arrays = g20
    x = sn.integer_input()
    with sd.installed():
        net = _rebuilt(ref)
        for switches, want in PARENT.items():
            kw = dict((s, True) for s in switches)
            got = resident.enable(net, x, **kw)
            assert got == want and list(got) == list(want), switches                     # the same keys, in the same order
            assert resident.enable(net, x, shuffle=False, **kw) == want
            plans = resident.describe(net)
            assert not plans.shuffle_left and all(p.perm is None for p in plans.values())
            if switches == ("depthwise", "concat"):
                assert sorted((n, p.emit_f32, p.emit_int, p.relu) for n, p in plans.items()) == PARENT_ROWS
            assert not any(isinstance(m.__dict__.get("forward"), resident._ShuffleResident) for m in net.modules())
            with torch.no_grad():
                net(x)
        assert not sd.calls


def test_with_flatten_a_concat_read_by_a_shuffle_is_launched_not_deferred(g20, monkeypatch):
    from common.quantity import resident
    ref, arrays = g20
    x = sn.integer_input()
    with sd.installed() as nat:
        net = _rebuilt(ref)
        on = resident.enable(net, x, flatten=True, **ON)
        plans = resident.describe(net)
        assert on["flattened_concats"] == 0 and plans.flattened_concats == () and not any(plans[c].defer for c in sn.CONCATS)
        launches = []
        real = nat.concat_i8_nhwc
        monkeypatch.setattr(nat, "concat_i8_nhwc", lambda srcs, relu, out=None: (launches.append(len(srcs)), real(srcs, relu, out))[1])
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
        assert launches == [2, 2, 2]


def test_the_full_width_model_keeps_every_unit_in_int8():
    """model/shufflenetv2/ShuffleNetV2_fabu.py at 1.0x (halves of 58, 116 and 232 channels) on 32 x 32 images without BatchNorm,
    seeded integer weights and fixed bits (shuffle_nets.unit_info): 16 shuffles, 26 slices, 16 Concats, and no fp32 output."""
    from common.quantity import resident
    x = sn.integer_input((2, 3, 32, 32))
    model = sn.integer_weights(sn.full_model(num_classes=10, width_mult=1.0, input_size=32, batch_norm=False)).eval()
    assert [model.units[k].shuffle.groups for k in (0, 15)] == [2, 2] and len(model.units) == 16
    assert [(u.left.start, u.left.stop, u.right.start, u.right.stop) for u in (model.units[1], model.units[5], model.units[13])] == \
        [(0, 58, 58, 116), (0, 116, 116, 232), (0, 232, 232, 464)]
    with sd.installed():
        net = dn.rebuild(model, sn.unit_info(model, x))
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, depthwise=True, concat=True)
        on = resident.enable(net, x, **ON)
        with torch.no_grad():
            assert torch.equal(net(x), plain) and float(plain.abs().max()) > 0
        assert on["resident_shuffles"] == 16 and on["resident_slices"] == 26 and on["resident_concats"] == 16
        assert on["fp32_outputs"] == 0 and off["fp32_outputs"] == 16 and not resident.describe(net).shuffle_left


def test_the_model_file_has_the_papers_widths():
    for mult, widths in ((0.5, (48, 96, 192, 1024)), (1.0, (116, 232, 464, 1024)), (1.5, (176, 352, 704, 1024)), (2.0, (244, 488, 976, 2048))):
        m = sn.full_model(num_classes=7, width_mult=mult, input_size=32)
        assert [len([u for u in m.units if u.Concat is not None])] == [16]
        assert (m.units[0].Concat is not None and m.conv1[0].out_channels == 24 and m.fc.in_features == widths[3]
                and m.conv5[0].in_channels == widths[2] and m.conv5[0].out_channels == widths[3])
        assert [m.units[k].branch[2][0].out_channels * 2 for k in (0, 4, 12)] == list(widths[:3])
        assert [m.units[k].down is not None for k in range(16)] == [k in (0, 4, 12) for k in range(16)]
        assert any(isinstance(mod, nn.BatchNorm2d) for mod in m.modules()) and not any(getattr(mod, "inplace", False) for mod in m.modules())
        with torch.no_grad():
            assert m.eval()(torch.zeros(1, 3, 32, 32)).shape == (1, 7)
    small = sn.full_model(num_classes=3, input_size=16, stages=(1, 2), widths=(12, 20, 32), batch_norm=False)
    assert len(small.units) == 3 and not any(isinstance(mod, nn.BatchNorm2d) for mod in small.modules())
    with torch.no_grad():
        assert small.eval()(torch.zeros(2, 3, 16, 16)).shape == (2, 3)


def test_random_units_keep_their_logits_under_the_plan():
    """The generator of scripts/recon_fuzz.py's `shuffle` mode (shuffle_nets.RandomShuffleNet: units cut anywhere, a shuffle or a
    slice alone, overlapping slices, a slice of a slice of a shuffle, every divisor as a group count) with fixed bits on the
    doubles: whatever the plan takes or leaves, the logits are the fp32-boundary model's, at the planned batch size and at one."""
    from common.quantity import resident
    total = {}
    with sd.installed():
        for i in range(16):
            m = sn.RandomShuffleNet(i, 5).eval()
            x = torch.randn(m.batch, 3, m.size, m.size, generator=torch.Generator().manual_seed(i))
            net = dn.rebuild(m, dn.fixed_info(m, out_bits=(3, 4), image_bit=4))
            with torch.no_grad():
                plain = net(x)
            on = resident.enable(net, x, flatten=True, **ON)
            with torch.no_grad():
                assert torch.equal(net(x), plain) and torch.equal(net(x[:1]), plain[:1]), (i, [s.kind for s in m.steps])
            left = resident.describe(net).shuffle_left
            hooked = sum(1 for mod in net.modules() if type(mod).__name__ in ("ChannelShuffle", "Slice"))
            assert on["resident_shuffles"] + on["resident_slices"] + len(left) == hooked, (i, on, left)
            for k, v in on.items():
                total[k] = total.get(k, 0) + v
        assert total["resident_shuffles"] > 3 and total["resident_slices"] > 10 and len(sd.calls) > 30, total


# ---------------------------------------------------------------- 3. what stays in fp32 form, and why
def _left(variant, **kw):
    from common.quantity import resident
    net = dn.seeded(sn.LeftNet(variant).eval())
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    model = dn.rebuild(net, dn.fixed_info(net, out_bits=(3, 4)))
    with torch.no_grad():
        plain = model(x)
    on = resident.enable(model, x, shuffle=True, **kw)
    with torch.no_grad():
        assert torch.equal(model(x), plain)
    return model, on, resident.describe(model)


def test_a_slice_of_a_newadd_sum_stays_fp32_and_describe_says_so():
    with sd.installed():
        _model, on, plans = _left("add")
        assert on["resident_slices"] == 0 and on["resident_adds"] == 1 and "sl" not in plans
        assert list(plans.shuffle_left) == ["sl"] and "NewAdd sum (int16)" in plans.shuffle_left["sl"]
        assert plans["Eltwise"].emit_f32 and not sd.calls


def test_a_shuffle_called_twice_stays_fp32_and_describe_says_so():
    with sd.installed():
        model, on, plans = _left("twice")
        assert on["resident_shuffles"] == 0 and "sh" not in plans
        assert list(plans.shuffle_left) == ["sh"] and "more than once" in plans.shuffle_left["sh"]
        assert plans["stem"].emit_f32 and "forward" not in model.sh.__dict__ and not sd.calls


def test_groups_that_do_not_divide_the_channels_are_refused_by_the_predicates():
    """torch's own module raises on such an input, so no forward can be traced: the two predicates the plan asks are held
    directly."""
    from common.quantity import _native, resident
    assert resident._shuffle_geometry(nn.ChannelShuffle(3), 20) is None and not _native.shuffle_supported(20, 0, 20, 3)
    assert resident._shuffle_geometry(nn.ChannelShuffle(4), 20) == (0, 20, 4) and _native.shuffle_supported(20, 0, 20, 4)
    for start, stop in ((0, 21), (-1, 5), (5, 5), (7, 3), (0.0, 5), (0, True), (None, 5)):
        assert resident._shuffle_geometry(sn.Slice(start, stop), 20) is None, (start, stop)
    assert resident._shuffle_geometry(sn.Slice(10, 20), 20) == (10, 10, 1)
    assert not _native.shuffle_supported(20, 0, 20, 1) and not _native.shuffle_supported(20, 0, 18, 1)      # nothing to do
    assert _native.shuffle_supported(20, 0, 16, 1) and _native.shuffle_supported(20, 1, 19, 1)


def test_a_bare_slice_stays_foreign_code():
    """Only the marker module is hooked: a bare x[:, a:b] -- like a slice along any other axis, a chunk or a split -- is a torch
    function at depth 0 and marks its source foreign, with and without the switch."""
    with sd.installed():
        _model, on, plans = _left("bare")
        assert on["resident_slices"] == 0 and on["resident_shuffles"] == 0 and not plans.shuffle_left
        assert plans["stem"].emit_f32 and not plans["stem"].emit_int and not sd.calls


def test_a_relu_directly_behind_a_shuffle_stays_torchs():
    from common.quantity import resident
    with sd.installed():
        model, on, plans = _left("relu")
        assert on["resident_shuffles"] == 1 and not plans.shuffle_left and len(sd.calls) == 2       # (verify + the forward in _left)
        p = plans["sh"]
        assert p.emit_f32 and not p.emit_int and not p.relu and p.perm == (0, 16, 4)
        assert not isinstance(model.r1.__dict__.get("forward"), resident._ReluPassThrough)
        assert plans["mid"].emit_int and not plans["mid"].emit_f32 and not plans["mid"].relu


def test_a_plan_pickled_before_the_slot_existed_still_loads():
    from common.quantity import resident
    p = resident.Plan()
    old = {k: v for k, v in p.__getstate__().items() if k != "perm"}
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(old)
    assert q.perm is None and q.__getstate__() == p.__getstate__()


# ---------------------------------------------------------------- 4. fq_shuffle_i8_nhwc: host arithmetic only
@pytest.fixture(scope="module")
def L():
    from common.quantity import _native
    return _native.lib()


@pytest.fixture(scope="module")
def buf():
    """(64-byte aligned pointer into a 4 KB host buffer filled with 0x55, a second one 2 KB behind it, the buffer)"""
    raw = ctypes.create_string_buffer(b"\x55" * (4096 + 64), 4096 + 64)
    base = (ctypes.addressof(raw) + 63) & ~63
    return ctypes.c_void_p(base), ctypes.c_void_p(base + 2048), raw


def _untouched(raw):
    return raw.raw == b"\x55" * (4096 + 64)


@no_gpu
def test_every_invalid_argument_is_refused_and_nothing_is_written(L, buf):
    p, p2, raw = buf
    # (x, Cpad_in, c_off, y, Cpad_out, C, groups, N, H, W)
    good = (p, 32, 10, p2, 16, 10, 1, 1, 2, 2)
    bad = {
        "null x": (None,) + good[1:], "null y": good[:3] + (None,) + good[4:],
        "misaligned x": (ctypes.c_void_p(p.value + 4),) + good[1:], "misaligned y": good[:3] + (ctypes.c_void_p(p2.value + 8),) + good[4:],
        "C < 1": (p, 32, 10, p2, 16, 0, 1, 1, 2, 2), "c_off < 0": (p, 32, -1, p2, 16, 10, 1, 1, 2, 2),
        "c_off + C > Cpad_in": (p, 32, 23, p2, 16, 10, 1, 1, 2, 2), "groups < 1": (p, 32, 10, p2, 16, 10, 0, 1, 2, 2),
        "C % groups": (p, 32, 10, p2, 16, 10, 3, 1, 2, 2), "Cpad_out": (p, 32, 10, p2, 32, 10, 1, 1, 2, 2),
        "nothing to do": (p, 64, 0, p2, 64, 64, 1, 1, 2, 2), "nothing to do, narrow": (p, 16, 0, p2, 16, 10, 1, 1, 2, 2),
        "N < 0": good[:7] + (-1, 2, 2), "H < 1": good[:7] + (1, 0, 2),
    }
    for what, a in bad.items():
        assert L.fq_shuffle_i8_nhwc(*a, None) == INVALID, what
    # N == 0 is FQ_OK, pointers or not; a scalar that is wrong is still refused
    assert L.fq_shuffle_i8_nhwc(None, 32, 10, None, 16, 10, 1, 0, 2, 2, None) == 0
    assert L.fq_shuffle_i8_nhwc(None, 32, 0, None, 32, 20, 2, 0, 2, 2, None) == 0
    assert L.fq_shuffle_i8_nhwc(None, 32, 10, None, 16, 10, 3, 0, 2, 2, None) == INVALID
    assert L.fq_shuffle_i8_nhwc(None, 64, 0, None, 64, 64, 1, 0, 2, 2, None) == INVALID
    assert _untouched(raw)


@no_gpu
def test_every_unsupported_geometry_is_refused_and_nothing_is_written(L, buf):
    p, p2, raw = buf
    assert L.fq_shuffle_i8_nhwc(p, 24, 2, p2, 16, 10, 1, 1, 2, 2, None) == UNSUPPORTED               # Cpad_in % 16
    assert L.fq_shuffle_i8_nhwc(p, 65568, 0, p2, 65552, 65540, 2, 1, 1, 1, None) == UNSUPPORTED      # C > 65536
    # the guard refuses a source or an output of 2^31 - 1 bytes or more.  Rows are multiples of 16 bytes and 2^31 - 1 is odd, so the
    # first total the guard can meet is 2^31 (2^31 - 16 would be admitted: nothing admitted is ever passed here, it would
    # launch)
    first = 1 << 31
    assert first - 16 < 0x7fffffff <= first
    assert L.fq_shuffle_i8_nhwc(p, 32, 10, p2, 16, 10, 1, first // 32 // 4, 2, 2, None) == UNSUPPORTED        # the source: 2^31 bytes
    assert L.fq_shuffle_i8_nhwc(p, 16, 0, p2, 16, 8, 2, first // 16 // 4, 2, 2, None) == UNSUPPORTED          # source and output
    assert L.fq_shuffle_i8_nhwc(p, 32, 0, p2, 32, 20, 2, first // 32, 1, 1, None) == UNSUPPORTED
    assert L.fq_shuffle_i8_nhwc(p, 16, 15, p2, 16, 1, 1, 1, 1 << 20, 1 << 20, None) == UNSUPPORTED            # N*H*W alone past 2^31
    assert L.fq_shuffle_i8_nhwc(p, 16, 15, p2, 16, 1, 1, 1 << 16, 1 << 16, 1 << 16, None) == UNSUPPORTED      # ... past 2^47
    assert _untouched(raw)


def test_supported_answers_on_both_sides_of_its_limits():
    from common.quantity import _native
    s = _native.shuffle_supported
    assert s(65536, 0, 65536, 2) and not s(65538, 0, 65538, 2) and s(65552, 16, 65536, 1) and not s(65553, 16, 65537, 1)
    assert s(116, 58, 58, 1) and s(116, 0, 58, 1) and s(116, 0, 116, 2) and s(244, 122, 122, 1) and s(18, 5, 13, 13)
    assert not s(116, 59, 58, 1) and not s(116, -1, 58, 1) and not s(116, 0, 0, 1) and not s(116, 0, 116, 0) and not s(116, 0, 116, 3)
    assert not s(0, 0, 1, 1) and s(1, 0, 1, 1) is False and s(17, 0, 1, 1) and s(6, 0, 6, 6)


# ---------------------------------------------------------------- 5. the kernel's address arithmetic on the host
def test_the_geometry_check_builds_and_passes_over_the_gpu_tests_shapes(tmp_path):
    """csrc/fq_shuffle_i8_geom.h compiled as host code with the address and undefined-behaviour sanitizers:
    scripts/shuffle_geom_check.cpp walks every stage item and every output byte of every launch and exits non-zero on an address
    outside its tensor, an unaligned 16-byte access, an output byte written twice or not at all, or a byte that is not the one
    the index rule names -- over its built-in list (both paths, tiles shortened by a wide span, the stride loop) and over the GPU
    tests' shape list."""
    exe = str(tmp_path / "shuffle_geom_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "shuffle_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,") and not out.stderr, out.stdout + out.stderr
    out = subprocess.run([exe] + [sn.case_arg(c) for c in sn.KERNEL_CASES], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(sn.KERNEL_CASES) + 1 and not out.stderr, \
        out.stdout + out.stderr
    rows = [re.match(r"case (\S+): lds (\d) tile (\d+) tiles (\d+) blocks (\d+)$", ln) for ln in lines[:-1]]
    assert all(rows)
    # every shape of the list runs the LDS path on tiles of sn.TILE pixels; the last one has one tile more than workgroups
    assert all(r.group(2) == "1" and int(r.group(3)) == sn.TILE for r in rows)
    assert (int(rows[-1].group(4)), int(rows[-1].group(5))) == (sn.MAX_BLOCKS + 1, sn.MAX_BLOCKS)
    assert max(int(r.group(4)) for r in rows[:-1]) == 2 and min(int(r.group(4)) for r in rows) == 1
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_shuffle_i8_geom.h")).read()
    assert re.search(r"kShufTilePix = %d;" % sn.TILE, header) and re.search(r"kShufMaxBlocks = %d;" % sn.MAX_BLOCKS, header)
