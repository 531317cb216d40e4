"""Elementwise activations that are no clamp (nn.LeakyReLU, nn.Hardswish, nn.SiLU, ...) in graph discovery, the tables and the
resident integer plan, on a box without a GPU: golden G21 (tests/golden/make_golden_activations.py) on the
oracle-backed engine, the 256-entry table against an elementwise evaluation, resident.enable(activations=True) on oracle-backed
doubles (tests/activation_doubles.py), what the lossy-value rule refuses and why, the host arithmetic of fq_act_lut_i8_nhwc, and
the kernel's index arithmetic walked on the host (scripts/act_lut_geom_check.cpp).  Every comparison is exact."""
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

import activation_doubles as ad
import activation_nets as an
import depthwise_nets as dn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, HIP, UNSUPPORTED = -1, -2, -4
ON = {"concat": True, "shuffle": True, "activations": True}
OFF = {"concat": True, "shuffle": True}
# resident.enable on the G21 net at the PARENT commit (2c1b75a), recorded by running that commit on the doubles of
# tests/shuffle_doubles.py: the summary per set of switches, and (emit_f32, emit_int, relu) of every planned module under
# concat=True, shuffle=True.  Every convolution in front of an activation leaves as fp32 there.
PARENT = {
    (): {"resident_convs": 4, "resident_adds": 0, "resident_pools": 1, "fused_relus": 1, "fp32_outputs": 3, "int_only_outputs": 1,
         "fused_conv_adds": 0, "fused_block_tails": 0, "fused_projections": 0},
    ("concat", "shuffle"): {"resident_convs": 4, "resident_adds": 0, "resident_pools": 1, "fused_relus": 1, "fp32_outputs": 3,
                            "int_only_outputs": 1, "resident_concats": 0, "resident_upsamples": 0, "resident_shuffles": 0,
                            "resident_slices": 0, "fused_conv_adds": 0, "fused_block_tails": 0, "fused_projections": 0,
                            "fused_upsamples": 0},
}
PARENT_ROWS = [("conv1", True, False, False), ("conv2", True, False, False), ("conv3", True, False, False),
               ("conv4", False, True, True)]


@pytest.fixture(scope="module")
def g21(golden_dir):
    with open(os.path.join(golden_dir, "g21_activation_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g21_activation_net.npz"))


def _x():
    return an.integer_input(an.G21_SHAPE, an.G21_INPUT_SEED)


def _rebuilt(ref):
    """g21_net as an integer-simulation model from the reference's own bits (ReconModel's module swap, depthwise_nets.rebuild)."""
    return dn.rebuild(an.integer_weights(an.g21_net()).eval(), copy.deepcopy(ref["quantity_information"]))


# ---------------------------------------------------------------- 1. settings, golden G21
def test_the_shipped_settings_list_the_names_and_the_header_declares_the_entry_points(g21):
    import yaml
    ref, _arrays = g21
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    assert ref["activation_names"] == list(an.ACTIVATIONS) and len(an.ACTIVATIONS) == 11
    # the golden decides: the shipped names are those the reference took through its whole flow -- all but PReLU
    assert ref["accepted_names"] == [n for n in an.ACTIVATIONS if n != "PReLU"] and "ok" not in ref["probe_graphs"]["PReLU"]["flow"]
    assert "PReLU" not in settings["ALL_OP_TYPE"] and "PReLU" not in settings["ALLOW_SAME_TID_OP_TYPE"]
    assert [n for n in settings["ALL_OP_TYPE"] if n in an.ACTIVATIONS] == ref["accepted_names"]
    for name in ref["accepted_names"]:
        assert name in settings["ALL_OP_TYPE"] and name in settings["ALLOW_SAME_TID_OP_TYPE"], name
        assert name not in settings["CARE_OP_TYPE"] and name not in settings["MERGE_OP_YTPE"]
        assert type(an.ACTIVATIONS[name]()).__name__ == name
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    assert re.search(r"^int fq_act_lut_i8_nhwc\(", text, re.M) and re.search(r"^int fq_act_lut_i8_nhwc_supported\(int C\);", text, re.M)
    from common.quantity import _native, resident
    assert _native.act_lut_supported(1) and _native.act_lut_supported(116) and not _native.act_lut_supported(0)
    assert set(t.__name__ for t in resident.ACTIVATION_TYPES) == set(an.ACTIVATIONS)
    assert not resident._is_table_activation(nn.ReLU6()) and not resident._is_table_activation(nn.ReLU())


def test_g21_activations_are_pruned_and_the_layer_behind_takes_the_bit_in_front(g21):
    ref, _arrays = g21
    info, q = ref["net_info"], ref["quantity_information"]
    assert not any(v["type"] in list(an.ACTIVATIONS) + ["Slice", "MaxPool2d"] for v in info.values())
    for probe in ref["probe_graphs"].values():                       # every listed type: conv -> activation -> conv
        first, second = probe["layers"]
        assert probe["inputs"] == {first: [], second: [first]}
    assert q["conv2"]["input_bit"] == q["conv1"]["output_bit"] and q["conv3"]["input_bit"] == q["Concat1"]["output_bit"]
    assert q["conv3"]["input_bit"] == q["conv4"]["input_bit"] == q["Concat2"]["output_bit"]


def test_g21_cpu_engine_matches_the_reference_and_the_plan_keeps_its_logits(g21, oracle):
    """The reference's graph discovery, merge groups, feat.table and both weight.tables byte for byte through the oracle-backed CPU
    engine on the SHIPPED settings, and its ReconModel logits bit for bit: plain, with the parent's switches and with
    activations=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g21
    shape = an.G21_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(an.integer_weights(an.g21_net()).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(an.integer_batches(3, shape, an.G21_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(an.integer_weights(an.g21_net()).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with ad.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = _x()
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                for kw in ({}, OFF, ON):
                    resident.enable(net, x, **kw)
                    np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"], err_msg=str(kw))
                    np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1], err_msg=str(kw))


# ---------------------------------------------------------------- 2. the table
@pytest.mark.parametrize("name", list(an.ACTIVATIONS))
def test_the_table_is_the_elementwise_chain_over_all_256_integers(name, oracle):
    m = an.ACTIVATIONS[name]().eval()
    before = copy.deepcopy(m.state_dict())
    for g, b in an.GRID_BIT_PAIRS:
        t = ad.build_act_table(m, g, b)
        assert t.dtype == torch.int8 and tuple(t.shape) == (256,)
        np.testing.assert_array_equal(t.numpy(), ad.elementwise_table(m, g, b), err_msg="%s (%d, %d)" % (name, g, b))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    if name in ("Sigmoid", "Hardsigmoid"):
        assert int(ad.build_act_table(m, 4, 7)[128]) == 64                # f(0) = 0.5: the table's entry for padding is not zero


def test_an_inplace_module_builds_its_table_on_a_fresh_tensor(oracle):
    a, b = nn.Hardswish(inplace=True), nn.Hardswish()
    assert torch.equal(ad.build_act_table(a, 4, 4), ad.build_act_table(b, 4, 4))


def test_the_kernels_double_zeroes_the_padding_whatever_the_table_holds():
    x = torch.from_numpy(np.random.default_rng(0).integers(-128, 128, (2, 3, 3, 16)).astype(np.int8))
    y = ad.act_lut_i8_nhwc(x, 5, torch.full((256,), 77, dtype=torch.int8))
    assert torch.all(y[..., :5] == 77) and torch.all(y[..., 5:] == 0)


# ---------------------------------------------------------------- 3. the plan on the doubles
def test_the_three_activations_are_planned_and_their_producers_emit_no_fp32(g21):
    from common.quantity import resident
    ref, arrays = g21
    x = _x()
    with ad.installed():
        net = _rebuilt(ref)
        with torch.no_grad():
            plain = net(x)
        np.testing.assert_array_equal(plain.numpy(), arrays["logits_recon"])
        off = resident.enable(net, x, **OFF)
        with torch.no_grad():
            off_logits = net(x)
        assert not ad.calls                                               # without the switch: no launch of the new entry point
        on = resident.enable(net, x, **ON)                               # verify=True: bit-identical to the traced forward
        plans = resident.describe(net)
        assert set(on) == set(off) | {"resident_activations"} and on["resident_activations"] == 3
        assert not plans.activations_left and plans.activations_revoked == ()
        q = ref["quantity_information"]
        for act, src, reader in (("act1", "conv1", "conv2"), ("act2", "conv2", "conv3"), ("act3", "conv3", "conv4")):
            p = plans[act]
            assert p.emit_int and not p.emit_f32 and not p.relu, (act, p)
            assert (p.grid, p.narrow_bit) == (q[src]["output_bit"], q[reader]["input_bit"])
            assert p.table.dtype == torch.int8 and p.table.numel() == 256
            assert torch.equal(p.table, ad.build_act_table(getattr(net, act), p.grid, p.narrow_bit))
            assert plans[src].emit_int and not plans[src].emit_f32 and not plans[src].relu, (src, plans[src])
        for name in ("pool", "left", "right", "Concat1", "up", "Concat2"):
            assert plans[name].emit_int and not plans[name].emit_f32, (name, plans[name])
        assert on["fp32_outputs"] == 0 and off["fp32_outputs"] == 3       # (conv4 hands its integers to the head's pool)
        assert all(p.table is None for n, p in plans.items() if n not in an.G21_ACTS)
        del ad.calls[:]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(got, off_logits) and torch.equal(net(x[:1]), plain[:1])
        np.testing.assert_array_equal(got.numpy(), arrays["logits_recon"])
        assert [c[0] for c in ad.calls] == [8, 12, 10, 8, 12, 10]
        buf = io.BytesIO()                                                # the plan, tables included, pickles with the model
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert torch.equal(resident.describe(again)["act2"].table, plans["act2"].table)
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and not resident.describe(net).activations_left
        with torch.no_grad():
            assert torch.equal(net(x), plain)


def test_without_the_switch_the_summary_and_the_plan_are_the_parents(g21):
    from common.quantity import resident
    ref, _arrays = g21
    x = _x()
    with ad.installed():
        net = _rebuilt(ref)
        for switches, want in PARENT.items():
            kw = dict((s, True) for s in switches)
            got = resident.enable(net, x, **kw)
            assert got == want and list(got) == list(want), switches                     # the same keys, in the same order
            assert resident.enable(net, x, activations=False, **kw) == want
            plans = resident.describe(net)
            assert not plans.activations_left and all(p.table is None for p in plans.values())
            assert sorted((n, p.emit_f32, p.emit_int, p.relu) for n, p in plans.items()) == PARENT_ROWS
            assert not any(isinstance(m.__dict__.get("forward"), resident._ActTableResident) for m in net.modules())
            with torch.no_grad():
                net(x)
        assert not ad.calls


# ---------------------------------------------------------------- 4. the lossy-value rule
REASONS = {"add": "read as fp32 by the NewAdd add", "avgpool": "read as fp32 by the average pool avg",
           "cat_grid": "revoked by the lossy rule: read as fp32 by cat", "bare_cat": "code outside the plan",
           "output": "model output", "two_bits": "different bits [3, 4]", "prelu_channels": "per-channel nn.PReLU",
           "twice": "more than once", "inplace": "inplace=True"}


def _refusal(variant, **kw):
    from common.quantity import resident
    model = an.RefusalNet(variant).eval()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    switches = dict(concat=True, avgpool=True)
    switches.update(kw)
    resident.enable(model, x, **switches)
    with torch.no_grad():
        off = [t.clone() for t in resident._iter_tensors(model(x))]
    on = resident.enable(model, x, activations=True, **switches)
    with torch.no_grad():
        got = list(resident._iter_tensors(model(x)))
    assert len(got) == len(off) and all(torch.equal(a, b) for a, b in zip(got, off))
    return model, on, resident.describe(model)


@pytest.mark.parametrize("variant", an.REFUSALS)
def test_what_the_rule_refuses_stays_torchs_with_its_reason_and_keeps_the_logits(variant):
    with ad.installed():
        model, on, plans = _refusal(variant)
        assert on["resident_activations"] == 0 and "act" not in plans and not ad.calls
        assert list(plans.activations_left) == ["act"] and REASONS[variant] in plans.activations_left["act"], plans.activations_left
        assert plans["mid"].emit_f32 and "forward" not in model.act.__dict__
        # only the Concat case was accepted by the first plan attempt and taken back by the verification
        assert plans.activations_revoked == (("act",) if variant == "cat_grid" else ())


def test_the_concat_case_passes_the_walk_and_fails_the_verification():
    from common.quantity import resident
    with ad.installed():
        model = an.RefusalNet("cat_grid").eval()
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
        switches = resident._switches(concat=True, activations=True)
        tracer, _out = resident._trace(model, x, switches)
        names = dict((m, n) for n, m in model.named_modules())
        first = resident._Planning(tracer, switches, names=names)
        first.plan_formats()
        first.plan_outputs()
        assert first.lossy == {model.act: 4} and first.plans[model.act].grid == 4                             # accepted (g, b) = (4, 4) ...
        assert not first.left["activations_left"] and model.act in first.plans
        assert model.cat not in first.int8_resident                                                           # ... the Concat is not
        assert first.verify() == {model.act: "revoked by the lossy rule: read as fp32 by cat"}
        second = resident._Planning(tracer, switches, revoked=first.verify(), names=names)
        second.plan_formats()
        second.plan_outputs()
        assert not second.lossy and not second.verify() and model.act not in second.plans


def test_the_same_net_with_the_operands_on_one_grid_is_planned_through_the_concat():
    from common.quantity import resident
    with ad.installed():
        model = an.RefusalNet("cat_grid").eval()
        model.other.output_bit = 4                         # (the other operand on the activation's grid)
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            plain = model(x)
        on = resident.enable(model, x, concat=True, activations=True)
        plans = resident.describe(model)
        assert on["resident_activations"] == 1 and on["resident_concats"] == 1 and not plans.activations_left
        assert not plans["act"].emit_f32 and not plans["cat"].emit_f32 and not plans["mid"].emit_f32
        with torch.no_grad():
            assert torch.equal(model(x), plain)


@pytest.mark.parametrize("name", list(an.ACTIVATIONS))
def test_every_listed_type_is_planned_between_two_convolutions(name):
    from common.quantity import resident
    with ad.installed():
        model = an.RefusalNet("ok", act=an.ACTIVATIONS[name]()).eval()
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))
        with torch.no_grad():
            plain = model(x)
        on = resident.enable(model, x, activations=True)
        assert on["resident_activations"] == 1 and not resident.describe(model).activations_left
        with torch.no_grad():
            assert torch.equal(model(x), plain)
        assert len(ad.calls) == 2                          # (verify + the forward above)


def test_random_nets_keep_their_logits_under_the_plan():
    """The generator of scripts/recon_fuzz.py's `act` mode (activation_nets.RandomActNet) with fixed bits on the doubles: whatever
    the plan takes or leaves, the logits are the fp32-boundary model's, at the planned batch size and at one."""
    from common.quantity import resident
    total = {}
    with ad.installed():
        for i in range(24):
            m = an.RandomActNet(i, 5).eval()
            x = torch.randn(m.batch, 3, m.size, m.size, generator=torch.Generator().manual_seed(i))
            net = dn.rebuild(m, dn.fixed_info(m, out_bits=(3, 4), image_bit=4))
            with torch.no_grad():
                plain = net(x)
            on = resident.enable(net, x, **ON)
            with torch.no_grad():
                assert torch.equal(net(x), plain) and torch.equal(net(x[:1]), plain[:1]), (i, m.steps)
            left = resident.describe(net).activations_left
            hooked = sum(1 for mod in net.modules() if resident._is_table_activation(mod))
            assert on["resident_activations"] + len(left) == hooked, (i, on, left)
            for k, v in on.items():
                total[k] = total.get(k, 0) + v
            total["left"] = total.get("left", 0) + len(left)
        assert total["resident_activations"] > 20 and total["left"] > 3 and len(ad.calls) > 60, total


def test_to_f32_on_a_lossy_handle_raises_and_the_movement_ops_pass_the_mark_on():
    from common.quantity import _native, resident
    q = torch.zeros(1, 4, 4, 16, dtype=torch.int8)
    h = resident.QHandle.int8(q, 8, 4, False)
    assert not h.lossy
    h.lossy = True
    with pytest.raises(_native.FqError, match="table activation"):
        h.to_f32()
    with pytest.raises(_native.FqError, match="table activation"):
        resident.as_f32(h)
    with ad.installed():
        pool = nn.MaxPool2d(2)
        pool.__dict__["_resident"] = plan = resident.Plan()
        plan.emit_f32, plan.emit_int = False, True
        out = resident._MaxPoolResident(pool)(h)
        assert type(out) is resident.QHandle and out.lossy
        h.lossy = False
        assert not resident._MaxPoolResident(pool)(h).lossy
        h.lossy = True
        up = resident.DeferredUpsample(h, 2)
        assert up.materialise().lossy
        cat = resident.DeferredConcat([(h, 1, False), (resident.QHandle.int8(q, 8, 4, False), 1, False)], 4)
        assert cat.materialise().lossy
        from common.quantity import NewAdd
        add = NewAdd()
        add.__dict__["_resident"] = p = resident.Plan()
        p.resident_add, p.grid, p.emit_int, p.emit_f32 = True, 4, True, False
        with pytest.raises(_native.FqError, match="table activation"):       # a sum of lossy integers is no sum of the values
            add(h, resident.QHandle.int8(q, 8, 4, False))


def test_a_plan_pickled_before_the_slot_existed_still_loads():
    from common.quantity import resident
    p = resident.Plan()
    old = {k: v for k, v in p.__getstate__().items() if k != "table"}
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(old)
    assert q.table is None and q.__getstate__() == p.__getstate__()


# ---------------------------------------------------------------- 5. fq_act_lut_i8_nhwc: host arithmetic only
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


@no_gpu
def test_null_pointers_and_non_positive_extents_are_invalid_arguments(L, buf):
    p, p2, raw = buf
    t = ctypes.c_void_p(p.value + 1024)
    good = (p, p2, t, 1, 2, 2, 10, 16)                     # (x, y, table, N, H, W, C, Cpad)
    bad = {"null x": (None,) + good[1:], "null y": good[:1] + (None,) + good[2:], "null table": good[:2] + (None,) + good[3:],
           "N = 0": good[:3] + (0, 2, 2, 10, 16), "N < 0": good[:3] + (-1, 2, 2, 10, 16), "H = 0": good[:3] + (1, 0, 2, 10, 16),
           "W < 0": good[:3] + (1, 2, -3, 10, 16), "C = 0": good[:3] + (1, 2, 2, 0, 16), "C < 0": good[:3] + (1, 2, 2, -1, 16),
           "Cpad < C": good[:3] + (1, 2, 2, 10, 8), "misaligned x": (ctypes.c_void_p(p.value + 4),) + good[1:],
           "misaligned y": good[:1] + (ctypes.c_void_p(p2.value + 8),) + good[2:]}
    for what, a in bad.items():
        assert L.fq_act_lut_i8_nhwc(*a, None) == INVALID, what
    assert raw.raw == b"\x55" * (4096 + 64)


@no_gpu
def test_one_byte_over_the_stated_limit_is_unsupported_and_the_limit_itself_passes_the_guard(L, buf):
    from common.quantity import _native
    p, p2, raw = buf
    t = ctypes.c_void_p(p.value + 1024)
    limit = _native.ACT_LUT_MAX_BYTES
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    assert limit == (1 << 31) - 2 and "N*H*W*Cpad > 2^31 - 2 bytes" in text
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_act_lut_i8_geom.h")).read()
    assert re.search(r"kActLutMaxBytes = 0x7ffffffeL;", header)
    assert limit % 2 == 0 and limit % 4 != 0
    over = [(1, 1, limit + 1, 1, 1), (1, limit // 2, 1, 2, 2 + 1), (limit // 2 + 1, 1, 1, 1, 2), (1 << 11, 1 << 10, 1 << 10, 1, 1),
            (1 << 16, 1 << 16, 1 << 16, 3, 16), (1, 1 << 20, 1 << 20, 1, 16)]
    for shape in over:
        assert L.fq_act_lut_i8_nhwc(p, p2, t, *shape, None) == UNSUPPORTED, shape
    # exactly the limit passes the guard: with no GPU the launch behind it fails, and that -- not a refusal -- is what comes back
    for shape in ((1, 1, limit, 1, 1), (1, limit // 2, 1, 2, 2), (limit // 2, 1, 1, 1, 2)):
        assert L.fq_act_lut_i8_nhwc(p, p2, t, *shape, None) == HIP, shape
    assert raw.raw == b"\x55" * (4096 + 64)


# ---------------------------------------------------------------- 6. the kernel's index arithmetic on the host
def test_the_geometry_check_builds_and_passes_over_the_gpu_tests_shapes(tmp_path):
    """csrc/fq_act_lut_i8_geom.h compiled as host code with the address and undefined-behaviour sanitizers:
    scripts/act_lut_geom_check.cpp walks every lane's chunks in every pass and the tail bytes and exits non-zero on an index
    outside the tensors or the table, an output byte written twice or not at all, or a byte that is not the one the rule names."""
    exe = str(tmp_path / "act_lut_geom_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "act_lut_geom_check.cpp")])
    out = subprocess.run([exe] + [an.case_arg(c) for c in an.KERNEL_CASES], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(an.KERNEL_CASES) + 1 and not out.stderr, \
        out.stdout + out.stderr
    rows = [re.match(r"case (\S+): chunks (\d+) tail (\d+) blocks (\d+) passes (\d+)$", ln) for ln in lines[:-1]]
    assert all(rows)
    assert (int(rows[-1].group(4)), int(rows[-1].group(5))) == (an.MAX_BLOCKS, 2)      # the stride loop runs twice
    assert all(int(r.group(5)) <= 1 for r in rows[:-1]) and any(int(r.group(3)) > 0 for r in rows) and any(r.group(2) == "0" for r in rows)
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_act_lut_i8_geom.h")).read()
    assert re.search(r"kActLutBlock = %d;" % an.BLOCK, header) and re.search(r"kActLutMaxBlocks = %d;" % an.MAX_BLOCKS, header)
