"""nn.PixelShuffle / nn.PixelUnshuffle in graph discovery, the tables and the resident integer plan, on a box without a GPU
(DESIGN section 32): golden G27 (tests/golden/make_golden_pixelshuffle.py) on the oracle-backed engine,
resident.enable(pixelshuffle=True) on oracle-backed doubles (tests/pixelshuffle_doubles.py: the index rule in numpy, held against
the reference's fp32 chain), what the plan leaves in fp32 form and why, the host arithmetic of fq_pixel_shuffle_i8_nhwc, and the
kernel's guards and address arithmetic walked on the host (scripts/pixel_shuffle_geom_check.cpp).  Every comparison is exact."""
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
import torch.nn.functional as F
from torch import nn

import activation_nets as an
import depthwise_nets as dn
import pixelshuffle_doubles as pd
import pixelshuffle_nets as pn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, UNSUPPORTED = -1, -4
ALL13 = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
             sums=True, topdown=True, bilinear=True, requant=True, pixelshuffle=True)
# resident.enable on the G27 net WITHOUT the switch: both modules are foreign code, conv1 and conv5 leave as fp32
G27_OFF = {"resident_convs": 6, "resident_adds": 1, "resident_pools": 0, "fused_relus": 3, "fp32_outputs": 3, "int_only_outputs": 4,
           "fused_conv_adds": 1, "fused_block_tails": 0, "fused_projections": 0}
G27_OFF_ROWS = [("Eltwise1", False, True, False), ("conv1", True, False, True), ("conv2", False, True, True),
                ("conv3", False, True, True), ("conv4", False, True, False), ("conv5", True, False, False),
                ("conv6", True, False, False)]


@pytest.fixture(scope="module")
def g27(golden_dir):
    with open(os.path.join(golden_dir, "g27_pixelshuffle_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g27_pixelshuffle_net.npz"))


def _rebuilt(ref):
    return dn.rebuild(an.integer_weights(pn.g27_net(), base_seed=pn.G27_SEED).eval(), copy.deepcopy(ref["quantity_information"]))


def _rows(plans):
    return sorted((n, p.emit_f32, p.emit_int, p.relu) for n, p in plans.items())


# ---------------------------------------------------------------- 1. the switch, the settings, the header, the model
def test_the_switch_is_accepted_and_off_by_default():
    """On the parent enable(pixelshuffle=True) is a TypeError."""
    import inspect
    from common.quantity import resident
    sig = inspect.signature(resident.enable)
    assert sig.parameters["pixelshuffle"].default is False
    with pd.installed():
        net = pn.ToyNet("conv_ps_conv").eval()
        on = resident.enable(net, pn.example(), pixelshuffle=True)
        assert on["resident_pixelshuffles"] == 1 and on["resident_pixelunshuffles"] == 0
        off = resident.enable(net, pn.example())
        assert "resident_pixelshuffles" not in off and "resident_pixelunshuffles" not in off


def test_the_settings_the_header_and_the_bindings_name_the_feature():
    import yaml
    from common.quantity import _native, resident
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    for name in ("PixelShuffle", "PixelUnshuffle"):
        assert name in settings["ALL_OP_TYPE"] and name in settings["ALLOW_SAME_TID_OP_TYPE"]
        assert name not in settings["CARE_OP_TYPE"] and name not in settings["MERGE_OP_YTPE"]
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    assert re.search(r"^int fq_pixel_shuffle_i8_nhwc\(const int8_t\* x, int Cpad_in, int8_t\* y, int Cpad_out, int C, int r, int inverse, "
                     r"int N, int H, int W,\s+fq_stream_t stream\);", text, re.M)
    assert re.search(r"^int fq_pixel_shuffle_i8_nhwc_supported\(int C, int r, int inverse\);", text, re.M)
    assert re.search(r"#define\s+FQ_VERSION\s+103\b", text) and _native.lib().fq_version() == 103
    L = _native.lib()
    assert L.fq_pixel_shuffle_i8_nhwc.restype is ctypes.c_int and len(L.fq_pixel_shuffle_i8_nhwc.argtypes) == 11
    assert len(L.fq_pixel_shuffle_i8_nhwc_supported.argtypes) == 3
    assert callable(_native.pixel_shuffle_supported) and callable(_native.pixel_shuffle_i8_nhwc)
    assert resident.Plan.__slots__ == ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer",
                                       "fuse_arg", "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip",
                                       "perm", "table")
    assert "pixelshuffle" in resident._MOVES and resident.describe(nn.Sequential()).pixelshuffle_left == {}


def test_edsr_imports_has_the_papers_shape_and_rejects_scale_5():
    for scale, factors in ((2, [2]), (3, [3]), (4, [2, 2])):
        m = pn.edsr_model(scale=scale, n_resblocks=2, n_feats=8).eval()
        ps = [mod for mod in m.modules() if isinstance(mod, nn.PixelShuffle)]
        assert [p.upscale_factor for p in ps] == factors
        assert [c.out_channels for c in m.upsampler if isinstance(c, nn.Conv2d)] == [8 * f * f for f in factors]
        assert sum(type(mod).__name__ == "Eltwise" for mod in m.modules()) == 3 and len(m.blocks) == 2
        assert not any(isinstance(mod, nn.BatchNorm2d) or getattr(mod, "inplace", False) for mod in m.modules())
        with torch.no_grad():
            assert m(torch.zeros(1, 3, 6, 5)).shape == (1, 3, 6 * scale, 5 * scale)
    full = pn.edsr_model()
    assert len(full.blocks) == 16 and full.head.out_channels == 64 and full.scale == 2
    for bad in (5, 1, 0, 8, "2"):
        with pytest.raises(ValueError):
            pn.edsr_model(scale=bad)


# ---------------------------------------------------------------- 2. the index rule
@pytest.mark.parametrize("r", pn.FACTORS)
def test_the_index_rule_is_torchs_pixel_shuffle_and_its_inverse(r):
    rng = np.random.default_rng(r)
    for C in (1, 3, 16, 17, 100):
        for (H, W) in ((1, 1), (2, 3), (5, 4)):
            deep = pn.source(rng, (2, H, W, C, r, 0))
            up = pn.pixel_rule(deep, C, r, 0)
            assert np.array_equal(up, pn.torch_rule(deep, C, r, 0)) and up.shape == (2, H * r, W * r, pn.pad16(C))
            assert not up[..., C:].any()
            t = torch.from_numpy(np.ascontiguousarray(deep[..., :C * r * r])).permute(0, 3, 1, 2)
            assert np.array_equal(up[..., :C], F.pixel_shuffle(t, r).permute(0, 2, 3, 1).numpy())
            back = pn.pixel_rule(up, C, r, 1)
            assert np.array_equal(back, pn.torch_rule(up, C, r, 1))
            assert np.array_equal(back[..., :C * r * r], deep[..., :C * r * r]) and not back[..., C * r * r:].any()     # the identity
            shal = pn.source(rng, (2, H, W, C, r, 1))
            assert np.array_equal(pn.pixel_rule(pn.pixel_rule(shal, C, r, 1), C, r, 0)[..., :C], shal[..., :C])


# ---------------------------------------------------------------- 3. host arithmetic only
def test_supported_answers_on_both_sides_of_its_limits():
    from common.quantity import _native
    s, fam = _native.pixel_shuffle_supported, _native.pixel_shuffle_family
    for inv in (0, 1):
        assert s(1, 2, inv) and s(3, 3, inv) and s(17, 4, inv) and s(100, 2, inv) and s(64, 2, inv)
        assert s(16384, 2, inv) and not s(16385, 2, inv) and s(4096, 4, inv) and not s(4097, 4, inv)
        assert s(7281, 3, inv) and not s(7282, 3, inv)
        assert not s(0, 2, inv) and not s(-1, 2, inv) and not s(16, 1, inv) and not s(16, 5, inv) and not s(16, 0, inv)
        for C in pn.KERNEL_CHANNELS:
            for r in pn.FACTORS:
                assert fam(C, r, inv) == pn.family(C, r)
    assert not s(16, 2, 2) and not s(16, 2, -1) and fam(16, 5, 0) == 0
    assert fam(16, 2, 0) == fam(64, 4, 1) == pn.ALIGNED and fam(16, 3, 0) == fam(17, 2, 0) == fam(3, 4, 1) == pn.GENERAL


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
def test_every_refusal_by_return_code_and_nothing_is_written(L, buf):
    p, p2, raw = buf
    f = L.fq_pixel_shuffle_i8_nhwc
    # (x, Cpad_in, y, Cpad_out, C, r, inverse, N, H, W)
    good = (p, 16, p2, 16, 3, 2, 0, 1, 2, 2)
    invalid = {
        "null x": (None,) + good[1:], "null y": good[:2] + (None,) + good[3:],
        "misaligned x": (ctypes.c_void_p(p.value + 4),) + good[1:], "misaligned y": good[:2] + (ctypes.c_void_p(p2.value + 8),) + good[3:],
        "N < 0": good[:7] + (-1, 2, 2), "H < 1": good[:7] + (1, 0, 2), "W < 1": good[:7] + (1, 2, 0), "C < 1": good[:4] + (0,) + good[5:],
        "inverse 2": good[:6] + (2,) + good[7:], "inverse -1": good[:6] + (-1,) + good[7:],
        "Cpad_in": (p, 32) + good[2:], "Cpad_out": good[:3] + (32,) + good[4:],
        "the other direction's Cpads": (p, 64, p2, 16, 16, 2, 1, 1, 2, 2),
    }
    for what, a in invalid.items():
        assert f(*a, None) == INVALID, what
    first = 1 << 31
    unsupported = {
        "r = 1": good[:5] + (1,) + good[6:], "r = 5": (p, 80, p2, 16, 3, 5, 0, 1, 2, 2), "r = 0": good[:5] + (0,) + good[6:],
        "C r^2 > 65536": (p, 65552, p2, 16400, 16385, 2, 0, 1, 1, 1),
        "an output of 2^31 bytes": good[:7] + (first // 16 // 4, 1, 1),
        "a source of 2^31 bytes": (p, 64, p2, 16, 16, 2, 0, first // 64, 1, 1),
        "N H W alone past 2^31": good[:7] + (1, 1 << 20, 1 << 20), "N H W past 2^47": good[:7] + (1 << 16, 1 << 16, 1 << 16),
    }
    for what, a in unsupported.items():
        assert f(*a, None) == UNSUPPORTED, what
    # scalars before pointers; N == 0 is FQ_OK without a launch, pointers or not, but a wrong scalar is still refused
    assert f(None, 16, None, 16, 3, 7, 0, 1, 2, 2, None) == UNSUPPORTED
    assert f(None, 16, None, 16, 3, 2, 0, 0, 2, 2, None) == 0 and f(None, 16, None, 64, 16, 2, 1, 0, 2, 2, None) == 0
    assert f(None, 32, None, 16, 3, 2, 0, 0, 2, 2, None) == INVALID and f(None, 16, None, 16, 3, 9, 0, 0, 2, 2, None) == UNSUPPORTED
    assert _untouched(raw)


# ---------------------------------------------------------------- 4. the kernel's guards and address arithmetic on the host
def test_the_walker_builds_with_the_sanitizers_and_passes(tmp_path):
    """csrc/fq_pixel_shuffle_i8_geom.h compiled as host code with the address and undefined-behaviour sanitizers:
    scripts/pixel_shuffle_geom_check.cpp checks the guard's table, then walks every lane of every launch -- every load inside its
    source and aligned, every output chunk written exactly once, the padding mask, every byte against the index rule -- over its
    built-in list, the GPU tests' two large launches and the model's launch shapes."""
    exe = str(tmp_path / "pixel_shuffle_geom_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "pixel_shuffle_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,") and not out.stderr, out.stdout + out.stderr
    small = [c for r in pn.FACTORS for inv in (0, 1) for c in pn.kernel_cases(r, inv) if c[:3] in ((1, 1, 1), (3, 5, 4))]
    cases = small + list(pn.BIG_CASES) + pn.model_launches()
    out = subprocess.run([exe] + [pn.case_arg(c) for c in cases], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(cases) + 1 and not out.stderr, out.stdout + out.stderr
    rows = [re.match(r"case (\S+): family (\d) items (\d+) blocks (\d+) passes (\d+)$", ln) for ln in lines[:-1]]
    assert all(rows)
    for c, row in zip(cases, rows):
        assert int(row.group(2)) == pn.family(c[3], c[4]), c
        assert int(row.group(4)) <= pn.MAX_BLOCKS
    big = rows[len(small):len(small) + 2]
    assert [int(b.group(2)) for b in big] == [pn.ALIGNED, pn.GENERAL] and all(int(b.group(5)) == 2 and int(b.group(4)) == pn.MAX_BLOCKS for b in big)
    assert all(int(row.group(5)) == 1 for row in rows[:len(small)])
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_pixel_shuffle_i8_geom.h")).read()
    assert re.search(r"kPsBlock = %d;" % pn.BLOCK, header) and re.search(r"kPsMaxBlocks = %d;" % pn.MAX_BLOCKS, header)


# ---------------------------------------------------------------- 5. what is planned
@pytest.mark.parametrize("variant", pn.TOY_VARIANTS)
def test_a_toy_net_is_planned_and_keeps_its_outputs(variant):
    from common.quantity import resident
    x = pn.example()
    with pd.installed():
        net = pn.ToyNet(variant).eval()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **net.kw)
        off_plans = resident.describe(net)
        with torch.no_grad():
            off_out = net(x)
        assert not pd.calls and "ps" not in off_plans and not off_plans.pixelshuffle_left
        for name in net.fronts:
            assert off_plans[name].emit_f32, name                              # the module is foreign code: its source leaves as fp32
        on = resident.enable(net, x, pixelshuffle=True, **net.kw)
        plans = resident.describe(net)
        C, r, inverse = net.launch
        assert set(on) == set(off) | {"resident_pixelshuffles", "resident_pixelunshuffles"} and not plans.pixelshuffle_left
        assert (on["resident_pixelshuffles"], on["resident_pixelunshuffles"]) == ((0, 1) if inverse else (1, 0))
        assert on["fp32_outputs"] < off["fp32_outputs"] or variant == "ps_out"
        for name in net.fronts:
            assert plans[name].emit_int and not plans[name].emit_f32, (name, plans[name])
        p = plans["ps"]
        assert p.up == r and p.perm == (("s2d" if inverse else "d2s"), C) and not p.relu
        assert (p.emit_f32, p.emit_int) == ((True, False) if variant == "ps_out" else (False, True))
        assert all(q.perm is None or n == "ps" for n, q in plans.items())
        if variant == "relu_ps":
            assert plans["a"].relu and isinstance(net.ra.__dict__.get("forward"), resident._ReluPassThrough)
        if variant == "act_ps":
            assert on["resident_activations"] == 1 and off["resident_activations"] == 0 and plans["act"].narrow_bit == 3
            assert p.narrow_bit == 3                                           # the lossy value walked through the module
        del pd.calls[:]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(got, off_out) and float(plain.abs().max()) > 0
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        assert [c[:3] for c in pd.calls] == [net.launch] * 3
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert resident.describe(again)["ps"].perm == p.perm
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and not resident.describe(net).pixelshuffle_left and "forward" not in net.ps.__dict__
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 6. what stays torch's, and why
@pytest.mark.parametrize("variant", sorted(pn.DECLINED))
def test_a_declined_module_stays_torchs_and_describe_says_why(variant, monkeypatch):
    from common.quantity import resident
    with pd.installed() as nat:
        net = pn.DeclinedNet(variant).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x)
        off_rows = _rows(resident.describe(net))
        if variant == "geometry":
            monkeypatch.setattr(nat, "pixel_shuffle_supported", lambda C, r, inverse: False)
        on = resident.enable(net, x, pixelshuffle=True)
        plans = resident.describe(net)
        assert on["resident_pixelshuffles"] == 0 and on["resident_pixelunshuffles"] == 0 and "ps" not in plans
        assert list(plans.pixelshuffle_left) == ["ps"] and pn.DECLINED[variant] in plans.pixelshuffle_left["ps"], plans.pixelshuffle_left
        assert _rows(plans) == off_rows and {k: v for k, v in on.items() if "pixel" not in k} == off       # the off arm's plan
        assert "forward" not in net.ps.__dict__ and not pd.calls
        with torch.no_grad():
            assert torch.equal(net(x), plain)


def test_the_ok_net_of_the_declined_family_is_planned():
    from common.quantity import resident
    with pd.installed():
        net = pn.DeclinedNet("ok").eval()
        on = resident.enable(net, net.example(), pixelshuffle=True)
        assert on["resident_pixelshuffles"] == 1 and not resident.describe(net).pixelshuffle_left


def test_the_geometry_predicate_refuses_what_the_kernel_would():
    from common.quantity import resident
    g = resident._pixel_geometry
    assert g(nn.PixelShuffle(2), (4, 32, 8, 8)) == (2, ("d2s", 8)) and g(nn.PixelUnshuffle(3), (1, 5, 6, 9)) == (3, ("s2d", 5))
    assert g(nn.PixelShuffle(2), (4, 30, 8, 8)) is None and g(nn.PixelUnshuffle(2), (4, 8, 7, 8)) is None
    assert g(nn.PixelShuffle(5), (4, 100, 8, 8)) is None and g(nn.PixelShuffle(2), (4, 32, 8)) is None
    for r in (2.0, True, None, "2"):
        m = nn.PixelShuffle(2)
        m.upscale_factor = r
        assert g(m, (4, 32, 8, 8)) is None, r


# ---------------------------------------------------------------- 7. switch off, pickling, run-time fallbacks
def test_without_the_switch_the_summary_and_the_plan_are_unchanged(g27):
    from common.quantity import resident
    ref, _arrays = g27
    x = an.integer_input(pn.G27_SHAPE, pn.G27_INPUT_SEED)
    with pd.installed():
        net = _rebuilt(ref)
        for kw in ({}, {"pixelshuffle": False}):
            got = resident.enable(net, x, **kw)
            assert got == G27_OFF and list(got) == list(G27_OFF), kw                 # the same keys, in the same order
            plans = resident.describe(net)
            assert _rows(plans) == G27_OFF_ROWS and not plans.pixelshuffle_left and all(p.perm is None for p in plans.values())
            assert not any(isinstance(m.__dict__.get("forward"), resident._PixelShuffleResident) for m in net.modules())
            with torch.no_grad():
                net(x)
        assert not pd.calls


def test_a_plan_pickled_before_the_feature_still_loads():
    from common.quantity import resident
    p = resident.Plan()
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(p.__getstate__())
    assert q.perm is None and q.up is None and q.__getstate__() == p.__getstate__()


def test_every_run_time_miss_falls_back_to_the_modules_own_forward(monkeypatch):
    from common.quantity import resident
    x = pn.example()
    with pd.installed() as nat:
        net = pn.ToyNet("conv_ps_conv").eval()
        resident.enable(net, x, pixelshuffle=True)
        ps = net.ps
        fwd = ps.__dict__["forward"]
        assert isinstance(fwd, resident._PixelShuffleResident)
        q = torch.randint(-128, 128, (2, 3, 5, 32), dtype=torch.int8)
        h = resident.QHandle.int8(q, 32, 4, False)
        want = F.pixel_shuffle(h.to_f32(), 2)
        del pd.calls[:]
        out = fwd(h)                                                           # the planned geometry: the kernel
        assert len(pd.calls) == 1 and torch.equal(resident.as_f32(out), want)
        del pd.calls[:]
        assert torch.equal(fwd(h.to_f32()), want)                              # an fp32 tensor without an integer form
        wide = resident.QHandle.wide_narrow(32, q.to(torch.int16), 4, None, None, False)
        assert torch.equal(fwd(wide), want)                                    # an int16 payload
        h48 = resident.QHandle.int8(torch.zeros(2, 3, 5, 48, dtype=torch.int8), 48, 4, False)
        assert fwd(h48).shape == (2, 12, 6, 10)                                # another width than the planned one
        ps.upscale_factor = 4
        assert torch.equal(fwd(h), F.pixel_shuffle(h.to_f32(), 4))             # another factor than the planned one
        ps.upscale_factor = 2
        monkeypatch.setattr(nat, "pixel_shuffle_supported", lambda C, r, inverse: False)
        assert torch.equal(fwd(h), want)                                       # a geometry the kernel refuses
        monkeypatch.undo()
        plan = ps.__dict__.pop("_resident")
        assert torch.equal(fwd(h), want)                                       # no plan
        ps.__dict__["_resident"] = plan
        assert not pd.calls
        assert torch.equal(resident.as_f32(fwd(h)), want) and len(pd.calls) == 1


# ---------------------------------------------------------------- 8. golden G27
def test_g27_both_modules_are_pruned_and_the_layer_behind_reads_at_the_bit_in_front(g27):
    ref, _arrays = g27
    info, q = ref["net_info"], ref["quantity_information"]
    assert not any(v["type"] in ("PixelShuffle", "PixelUnshuffle") for v in info.values())
    assert sum(v["type"] == "Conv2d" for v in info.values()) == 6 and sum(v["type"] == "Eltwise" for v in info.values()) == 1
    assert q["conv2"]["input_bit"] == q["conv1"]["output_bit"] and q["conv6"]["input_bit"] == q["conv5"]["output_bit"]


def test_g27_cpu_engine_matches_the_reference_and_the_plan_keeps_its_logits(g27, oracle):
    """The reference's graph discovery, merge groups, feat.table and both weight.tables of the G27 net byte for byte through the
    oracle-backed CPU engine on the SHIPPED settings (on the parent discovery stops at the layer behind the first module), and its
    ReconModel logits bit for bit: plain, with the switch off, on, and with all thirteen."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g27
    shape = pn.G27_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(an.integer_weights(pn.g27_net(), base_seed=pn.G27_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(an.integer_batches(3, shape, pn.G27_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(an.integer_weights(pn.g27_net(), base_seed=pn.G27_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with pd.installed_all():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = an.integer_input(shape, pn.G27_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                for kw in ({}, {"pixelshuffle": True}, ALL13):
                    summary = resident.enable(net, x, **kw)
                    np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"], err_msg=str(kw))
                    np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1], err_msg=str(kw))
                    if kw:
                        assert summary["resident_pixelshuffles"] == 1 and summary["resident_pixelunshuffles"] == 1
                        plans = resident.describe(net)
                        assert not plans.pixelshuffle_left and plans["unshuffle"].perm == ("s2d", 8) and plans["shuffle"].perm == ("d2s", 8)
                        assert not plans["conv1"].emit_f32 and not plans["conv5"].emit_f32 and summary["fp32_outputs"] == 1


# ---------------------------------------------------------------- 9. the random family
def test_forty_random_nets_keep_their_outputs_under_the_switch_alone_and_under_all_thirteen():
    """Whatever the plan takes or leaves, the outputs are the fp32-boundary model's, at the planned batch size and at one.  At least
    80 % of the drawn modules are planned, and each direction and each factor at least ten times (the generator's seeds are chosen
    so; the counts are printed)."""
    from common.quantity import resident
    drawn = planned = 0
    by = {}
    with pd.installed_all():
        for seed in pn.SEEDS:
            m = pn.RandomPixelShuffleNet(seed).eval()
            x = m.example()
            with torch.no_grad():
                plain = m(x)
            for kw in ({"pixelshuffle": True}, ALL13):
                on = resident.enable(m, x, **kw)
                with torch.no_grad():
                    assert torch.equal(m(x), plain) and torch.equal(m(x[:1]), plain[:1]), (seed, kw, [s["kind"] for s in m.stages])
                plans = resident.describe(m)
                left = plans.pixelshuffle_left
                assert on["resident_pixelshuffles"] + on["resident_pixelunshuffles"] + len(left) == len(m.mods_drawn), (seed, on, left)
                for name, way, r, expected in m.mods_drawn:
                    assert (name in plans) == expected and (name in left) != expected, (seed, name, left)
            for name, way, r, expected in m.mods_drawn:
                drawn += 1
                if name in plans:
                    planned += 1
                    by[way] = by.get(way, 0) + 1
                    by[r] = by.get(r, 0) + 1
            resident.disable(m)
    print("random pixel-shuffle nets: %d modules drawn, %d planned, by direction and factor %s" % (drawn, planned, sorted(by.items(), key=str)))
    assert planned >= 0.8 * drawn
    assert all(by.get(k, 0) >= 10 for k in ("ps", "pu", 2, 3, 4)), by
