"""resident.enable(..., concat=True, requant=True) and its kernel's contract (fq_concat_rq_i8_nhwc) on a box without a GPU.

The closed form (requant_ref.py) is held against the reference's literal chain -- the oracle's DeQuantity, torch.cat, ReLU, the
oracle's Quantity -- for every int8 and int16 value; the plan runs on doubles that take that chain literally (requant_doubles.py);
the kernel's index arithmetic, its rounding and its guards are walked on the host (scripts/concat_geom_check.cpp); golden G26
pins a calibrated net with a residual skip to the reference; forty random nets run under three plans.  Every comparison is exact."""
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

import activation_nets as an
import mixed_nets as mn
import requant_doubles as rd
import requant_nets as rn
import requant_ref as rr
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, HIP, UNSUPPORTED = -1, -2, -4
OFF = dict(concat=True)
ON = dict(concat=True, requant=True)
ALL_TWELVE = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
                  sums=True, topdown=True, bilinear=True, requant=True)
SLOTS = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg", "fuse_next",
         "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip", "perm", "table")
NEW_KEYS = {"requant_concats", "requant_sum_sources"}


def _plans(model):
    from common.quantity import resident
    return resident.describe(model)


def _rows(model):
    def plain(v):
        return tuple(v.tolist()) if isinstance(v, torch.Tensor) else v
    return {n: tuple(plain(getattr(p, f)) for f in p.__slots__) for n, p in _plans(model).items()}


def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def _same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _check_forwards(net, x, plain):
    """the example, one image, a flipped batch"""
    with torch.no_grad():
        assert _same(net(x), plain)
        assert _same(net(x[:1]), tuple(p[:1] for p in _tuple(plain)))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in _tuple(plain)))


def _without(summary):
    return {k: v for k, v in summary.items() if k not in NEW_KEYS}


# ---------------------------------------------------------------- 1. the closed form against the literal chain
@pytest.mark.parametrize("wide", (False, True), ids=("int8", "int16"))
def test_the_closed_form_is_the_literal_chain_on_every_value(wide, oracle):
    """All 256 int8 / all 65 536 int16 values as one source of 256 channels (int16: a 16 x 16 plane of them), joined with a second
    int8 source on another grid, every shift in [-8, 8], ReLU on and off, upsampling 1, 2 and 4."""
    if wide:
        a = np.arange(-32768, 32768).astype(np.int16).reshape(1, 16, 16, 256)
    else:
        a = np.broadcast_to(np.arange(-128, 128).astype(np.int8)[None, None, None, :], (1, 4, 4, 256)).copy()
    ties = 0
    for up in (1, 2, 4):
        other = np.random.default_rng(up).integers(-128, 128, (1, a.shape[1] * up, a.shape[2] * up, 16)).astype(np.int8)
        for shift in range(-8, 9):
            for relu in (False, True):
                for g in (0, 3):
                    want = rd.literal_chain([(a, 256, up, relu, g), (other, 5, 1, relu, g + shift + 1)], g + shift)
                    got = rr.concat_rq([(a, 256, up, relu, shift), (other, 5, 1, relu, -1)])
                    np.testing.assert_array_equal(got[..., :261], want, err_msg=str((up, shift, relu, g)))
                    assert not got[..., 261:].any()
            ties += rr.ties(a, shift)
    print("closed form, %s: %d exact ties met" % ("int16" if wide else "int8", ties))
    assert ties == 3 * (a.size // 256) * 255                       # (one value in 2^k at shift -k: the half-to-even branch is walked at every negative shift)


def test_the_double_zeroes_the_padding_and_depends_on_the_shift_alone(oracle):
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(-32768, 32768, (2, 3, 5, 32)).astype(np.int16))
    z = torch.from_numpy(rng.integers(-128, 128, (2, 6, 10, 16)).astype(np.int8))
    y = rd.concat_rq_i8_nhwc([(x, 19, 2, True, -7), (z, 3, 1, False, 1)])
    assert tuple(y.shape) == (2, 6, 10, 32) and not y[..., 22:].any() and int(y[..., :19].min()) == 0 and int(y[..., 19:22].min()) < 0
    np.testing.assert_array_equal(y.numpy(), rr.concat_rq([(x.numpy(), 19, 2, True, -7), (z.numpy(), 3, 1, False, 1)]))
    assert rd.calls[-1] == [(19, 2, 2, True, -7), (3, 1, 1, False, 1)]


# ---------------------------------------------------------------- 2. the switch, the entry points
def test_requant_is_accepted_and_needs_concat():
    from common.quantity import resident
    with rd.installed():
        net = rn.ToyNet("two_grids").eval()
        for kw in (dict(requant=True), dict(requant=True, concat=False), dict(requant=True, shuffle=True, activations=True)):
            with pytest.raises(ValueError, match="concat=True"):
                resident.enable(net, rn.example(), **kw)
        assert not resident.is_enabled(net)
        assert resident.enable(net, rn.example(), **ON)["requant_concats"] == 1


def test_the_binding_and_the_header_symbol_exist():
    from common.quantity import _native
    assert callable(_native.concat_rq_i8_nhwc) and callable(_native.concat_rq_supported)
    with open(os.path.join(ROOT, "include", "fq.h")) as fh:
        text = fh.read()
    assert re.search(r"^typedef struct fq_cat_src_rq \{ const void\* q; int bytes; int C; int Cpad; int up; int relu; int shift; \} fq_cat_src_rq;",
                     text, re.M)
    assert re.search(r"^int fq_concat_rq_i8_nhwc_supported\(const int\* C, const int\* up, const int\* bytes, const int\* shift, int nsrc\);", text, re.M)
    assert re.search(r"^int fq_concat_rq_i8_nhwc\(const fq_cat_src_rq\* srcs, int nsrc, int8_t\* out, int Cpad_out, int N, int H, int W,", text, re.M)
    L = _native.lib()
    assert L.fq_concat_rq_i8_nhwc.restype is ctypes.c_int and len(L.fq_concat_rq_i8_nhwc.argtypes) == 8
    assert ctypes.sizeof(_native._CatSrcRq) == 32 and _native._CatSrcRq.shift.offset == 28


def test_resunet_imports_and_checks_its_input_size():
    for size in (0, 16, 48, 225):
        with pytest.raises(ValueError):
            rn.resunet_model(input_size=size)
    m = rn.resunet_model(num_classes=3, input_size=32, base_width=8, layers=(1, 1, 1, 1), batch_norm=False).eval()
    assert sum(type(mod).__name__ == "Concat" for mod in m.modules()) == 3 and sum(type(mod).__name__ == "Eltwise" for mod in m.modules()) == 4
    ups = [mod for mod in m.modules() if isinstance(mod, nn.Upsample)]
    assert len(ups) == 3 and all(u.mode == "bilinear" and not u.align_corners and u.scale_factor == 2 for u in ups)
    with torch.no_grad():
        assert tuple(m(rn.example(2, 32)).shape) == (2, 3, 8, 8)
    assert sum(type(mod).__name__ == "Eltwise" for mod in rn.resunet_model(input_size=32, base_width=4).modules()) == 8


def test_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.concat_rq_supported
    for shift in range(-12, 13):
        for by in (0, 1, 2, 3):
            for up in (0, 1, 2, 3, 4, 8):
                assert ok([16, 3], [1, up], [by, 1], [shift, 0]) == (abs(shift) <= 8 and by in (1, 2) and up in (1, 2, 4)), (shift, by, up)
    assert ok([1], [1], [1], [0]) and ok([16] * 8, [1] * 8, [2] * 8, [8] * 8) and not ok([16] * 9, [1] * 9, [1] * 9, [0] * 9)
    assert not ok([], [], [], []) and not ok([0, 16], [1, 1], [1, 1], [0, 0]) and not ok([16, 16], [1], [1, 1], [0, 0])
    assert ok([65536], [1], [1], [1]) and not ok([65536, 1], [1, 1], [1, 1], [0, 0]) and not ok([65537], [1], [1], [0])


@pytest.fixture(scope="module")
def L():
    from common.quantity import _native
    return _native.lib()


@pytest.fixture(scope="module")
def buf():
    """(64-byte aligned pointers 0, 1 KB and 2 KB into a 4 KB host buffer filled with 0x55, the buffer)"""
    raw = ctypes.create_string_buffer(b"\x55" * (4096 + 64), 4096 + 64)
    base = (ctypes.addressof(raw) + 63) & ~63
    return base, base + 1024, base + 2048, raw


def _call(L, srcs, nsrc, out, cpad_out, N, H, W):
    from common.quantity import _native
    arr = (_native._CatSrcRq * max(len(srcs), 1))()
    for i, (q, by, C, cpad, up, relu, shift) in enumerate(srcs):
        arr[i].q, arr[i].bytes, arr[i].C, arr[i].Cpad, arr[i].up, arr[i].relu, arr[i].shift = q, by, C, cpad, up, relu, shift
    return L.fq_concat_rq_i8_nhwc(arr, nsrc, ctypes.c_void_p(out) if out is not None else None, cpad_out, N, H, W, None)


@no_gpu
def test_the_host_side_guards_and_their_return_codes(L, buf):
    p0, p1, p2, raw = buf
    A, B = (p0, 1, 16, 16, 1, 0, -3), (p1, 2, 16, 16, 1, 1, 2)           # (q, bytes, C, Cpad, up, relu, shift)

    def a_(**kw):
        names = ("q", "bytes", "C", "Cpad", "up", "relu", "shift")
        return tuple(kw.get(n, v) for n, v in zip(names, A))

    assert L.fq_concat_rq_i8_nhwc(None, 2, ctypes.c_void_p(p2), 32, 1, 2, 2, None) == INVALID
    invalid = {"nsrc 0": ([A, B], 0, p2, 32, 1, 2, 2), "nsrc -1": ([A, B], -1, p2, 32, 1, 2, 2), "no output": ([A, B], 2, None, 32, 1, 2, 2),
               "misaligned output": ([A, B], 2, p2 + 8, 32, 1, 2, 2), "no source": ([a_(q=None), B], 2, p2, 32, 1, 2, 2),
               "misaligned source": ([a_(q=p0 + 4), B], 2, p2, 32, 1, 2, 2), "C 0": ([a_(C=0), B], 2, p2, 16, 1, 2, 2),
               "up 0": ([a_(up=0), B], 2, p2, 32, 1, 2, 2), "Cpad < C": ([a_(Cpad=8), B], 2, p2, 32, 1, 2, 2),
               "relu 2": ([a_(relu=2), B], 2, p2, 32, 1, 2, 2), "relu -1": ([a_(relu=-1), B], 2, p2, 32, 1, 2, 2),
               "bytes 0": ([a_(bytes=0), B], 2, p2, 32, 1, 2, 2), "bytes 3": ([a_(bytes=3), B], 2, p2, 32, 1, 2, 2),
               "bytes 4": ([a_(bytes=4), B], 2, p2, 32, 1, 2, 2), "Cpad_out": ([A, B], 2, p2, 48, 1, 2, 2),
               "N < 0": ([A, B], 2, p2, 32, -1, 2, 2), "H 0": ([A, B], 2, p2, 32, 1, 0, 2), "W < 0": ([A, B], 2, p2, 32, 1, 2, -2),
               "nothing to do": ([a_(shift=0)], 1, p2, 16, 1, 2, 2)}
    for what, args in invalid.items():
        assert _call(L, *args) == INVALID, what
    unsupported = {"nine sources": ([A] * 9, 9, p2, 144, 1, 2, 2), "shift 9": ([a_(shift=9), B], 2, p2, 32, 1, 2, 2),
                   "shift -9": ([a_(shift=-9), B], 2, p2, 32, 1, 2, 2), "up 3": ([a_(up=3), B], 2, p2, 32, 1, 6, 6),
                   "up 8": ([a_(up=8), B], 2, p2, 32, 1, 8, 8), "H % up": ([a_(up=2), B], 2, p2, 32, 1, 3, 2),
                   "W % up": ([A, (p1, 2, 16, 16, 4, 1, 2)], 2, p2, 32, 1, 4, 6), "Cpad % 16": ([a_(Cpad=24), B], 2, p2, 32, 1, 2, 2),
                   "sum C > 65536": ([a_(C=65536, Cpad=65536), B], 2, p2, 65552, 1, 1, 1),
                   "2^31 bytes out": ([A, B], 2, p2, 32, 1, 8192, 8192), "far over": ([A, B], 2, p2, 32, 1 << 30, 1 << 30, 1 << 30),
                   "an int16 source of 2^31 bytes": ([(p0, 1, 1, 16, 1, 0, 1), (p1, 2, 16, 1024, 1, 0, 0)], 2, p2, 32, 1, 1024, 1024)}
    for what, args in unsupported.items():
        assert _call(L, *args) == UNSUPPORTED, what
    # an invalid argument is named before an unsupported one; N == 0 is fine whatever the pointers and the other sizes are
    assert _call(L, [a_(C=0, shift=9), B], 2, p2, 16, 1, 2, 2) == INVALID
    assert _call(L, [a_(q=None), (None, 2, 16, 16, 1, 1, 2)], 2, None, 32, 0, 1 << 20, 1 << 20) == 0
    assert _call(L, [a_(shift=9), B], 2, p2, 32, 0, 2, 2) == UNSUPPORTED
    # what passes the guards is launched: with no GPU the launch fails, and that -- not a refusal -- is what comes back
    for args in (([A, B], 2, p2, 32, 1, 2, 2), ([a_(shift=0, relu=1)], 1, p2, 16, 1, 2, 2), ([(p1, 2, 16, 16, 1, 0, 0)], 1, p2, 16, 1, 2, 2),
                 ([a_(shift=1)], 1, p2, 16, 1, 2, 2), ([a_(shift=0, up=2)], 1, p2, 16, 1, 2, 2), ([a_(shift=8), (p1, 2, 3, 16, 1, 1, -8)], 2, p2, 32, 1, 2, 2)):
        assert _call(L, *args) == HIP, args
    assert raw.raw == b"\x55" * (4096 + 64)
    # just under the limits (pointers that are never touched: the launch fails first)
    big = 1 << 44
    assert _call(L, [A, B], 2, big, 32, 1, 8192, 8191) == HIP
    assert _call(L, [(p0, 1, 1, 16, 1, 0, 1), (big, 1, 16, 1024, 1, 0, 0)], 2, big * 2, 32, 1, 1024, 1024) == HIP     # (the same source as int8)


# ---------------------------------------------------------------- 3. the walker
def test_kernel_address_arithmetic_rounding_and_guards_on_the_host(tmp_path):
    """csrc/fq_concat_i8_geom.h holds the kernel's lane -> (sources, offsets, masks, loads) functions, its rounding and its
    guards, and compiles as host code: scripts/concat_geom_check.cpp, built with the address and undefined-behaviour sanitizers,
    walks every lane of every launch of the GPU tests' cases and of the two models' launch shapes."""
    exe = str(tmp_path / "concat_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "concat_geom_check.cpp")])
    cases = [c for n in rn.KERNEL_NSRC for p in rn.KERNEL_PLANES for c in rn.kernel_cases(n, p)] + [rn.BIG_CASE] + rn.model_launches()
    args = sorted(set(rn.case_arg(c) for c in cases))
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(args) + 3 and not out.stderr, out.stdout[-2000:] + out.stderr
    assert lines[-3].startswith("requant: %d values" % (17 * 2 * 65536)) and lines[-2].startswith("guards:")
    assert int(lines[-3].split()[-2]) == 2 * sum(65536 >> 1 >> (k - 1) for k in range(1, 9))      # (ties: odd multiples of 2^(k-1))
    row = {ln.split(":")[0][5:]: ln.split() for ln in lines if ln.startswith("case ")}
    big = row[rn.case_arg(rn.BIG_CASE)]
    assert int(big[big.index("chunks") + 1]) == 3 * 120 * 120 * 13 > 2048 * 256 and int(big[big.index("blocks") + 1]) == 2048
    assert int(big[big.index("second-items") + 1]) > 0 and int(big[big.index("general") + 1]) > 0
    for c in rn.model_launches():                                 # what models hit: the aligned family only
        r = row[rn.case_arg(c)]
        assert int(r[r.index("general") + 1]) == 0, r
    mixed = [row[rn.case_arg(c)] for c in rn.kernel_cases(8, (8, 8)) if c[3] == (1, 3, 16, 19, 33, 100, 1, 3)]
    assert len(mixed) == 10 and all(int(r[r.index("general") + 1]) > 0 for r in mixed)       # (int16 sources at unaligned channel offsets)
    for bad in ("1,4,4/16/3/1", "1,4,4/16,16/1,1/1,3", "1,5,4/16/2/1", "1,4,4/16"):
        assert subprocess.run([exe, bad], capture_output=True, text=True).returncode in (1, 2), bad
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_concat_i8_geom.h")).read()
    assert re.search(r"kCrqMaxSrc = 8;", header) and re.search(r"kCrqMaxShift = 8;", header) and re.search(r"kCrqMaxBytes = 0x7ffffffeL;", header)


def test_int8_sources_at_shift_0_are_the_moving_concat_on_the_doubles():
    """The identity tests/test_gpu_concat_rq_i8.py holds the kernels to, on the two doubles."""
    import concat_n_doubles
    from test_gpu_concat_rq_i8 import IDENTITY_CASES
    for N, H, W, Cs, ups, relus in IDENTITY_CASES:
        arrays = rn.sources(np.random.default_rng(sum(Cs)), (N, H, W, Cs, ups, (1,) * len(Cs), (0,) * len(Cs), relus))
        qs = [torch.from_numpy(a) for a in arrays]
        moved = concat_n_doubles.concat_n_i8_nhwc([(q, C, up, relu) for q, C, up, relu in zip(qs, Cs, ups, relus)])
        assert torch.equal(moved, rd.concat_rq_i8_nhwc([(q, C, up, relu, 0) for q, C, up, relu in zip(qs, Cs, ups, relus)]))


def test_the_gpu_tests_case_list_meets_every_value_it_claims():
    cases = [c for n in rn.KERNEL_NSRC for p in rn.KERNEL_PLANES for c in rn.kernel_cases(n, p)]
    assert set(c[0] for c in cases) == set(rn.KERNEL_N) and set(len(c[3]) for c in cases) == set(rn.KERNEL_NSRC)
    assert set(ch for c in cases for ch in c[3]) == set(rn.KERNEL_CHANNELS)
    assert set(u for c in cases for u in c[4]) == set(rn.KERNEL_UPS) and set(s for c in cases for s in c[6]) == set(rn.KERNEL_SHIFTS)
    for n in (1, 2, 3):                                                     # every int8 / int16 mix, both ReLU flags in every position
        assert set(c[5] for c in cases if len(c[3]) == n) == set(tuple(int(b) + 1 for b in format(i, "0%db" % n)) for i in range(2 ** n))
        assert set(c[7] for c in cases if len(c[3]) == n) >= set(tuple(int(b) for b in format(i, "0%db" % n)) for i in range(2 ** n))
    wide_unaligned = [c for c in cases if any(b == 2 and sum(c[3][:i]) % 16 for i, b in enumerate(c[5]))]
    assert len(wide_unaligned) > 50                                         # int16 sources that start at an unaligned channel offset


# ---------------------------------------------------------------- 4. what is planned
@pytest.mark.parametrize("variant", rn.TOY_VARIANTS)
def test_one_toy_net_per_cause(variant):
    """The Concat is one launch of the new entry point with the expected sources, the producers in front of it go from emit_f32 to
    integers only, and on == off == plain on the example, on one image and on a flipped batch."""
    from common.quantity import resident
    with rd.installed():
        net = rn.ToyNet(variant).eval()
        x = rn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **dict(OFF, **net.kw))
        off_plans = _plans(net)
        _check_forwards(net, x, plain)
        assert not NEW_KEYS & set(off) and not rd.calls and not off_plans.requant_left
        assert all(off_plans[f].emit_f32 for f in net.fronts), {f: off_plans[f] for f in net.fronts}
        on = resident.enable(net, x, **dict(ON, **net.kw))
        plans = _plans(net)
        assert set(on) == set(off) | NEW_KEYS and on["requant_concats"] == 1 and not plans.requant_left, (on, plans.requant_left)
        assert on["requant_sum_sources"] == (1 if variant in ("sum", "sum_relu") else 0)
        del rd.calls[:]
        _check_forwards(net, x, plain)
        assert rd.calls == [net.launch] * 3, rd.calls
        for f in net.fronts:
            assert plans[f].emit_int and not plans[f].emit_f32, (f, plans[f])
        p = plans["cat"]
        assert p.emit_int and not p.emit_f32 and type(p.grid) is tuple and len(p.grid) == 2 and not p.defer
        assert p.narrow_bit == net.head.input_bit and [p.narrow_bit - g for g in p.grid] == [s[4] for s in net.launch]
        assert isinstance(net.cat.__dict__.get("forward"), resident._ConcatRequant)
        assert on["fp32_outputs"] < off["fp32_outputs"] and on["resident_concats"] == 1
        if variant in ("sum", "sum_relu"):
            assert plans["add"].want_wide and plans["add"].resident_add and plans["add"].relu == (variant == "sum_relu")
            assert not off_plans["add"].emit_int or off_plans["add"].emit_f32
        if variant == "upsampled":
            assert plans["up"].defer and on["fused_upsamples"] == 1
        if variant == "bilinear":
            assert off["resident_bilinears"] == 0 and "revoked by the lossy rule: read as fp32 by cat" in off_plans.bilinear_left["up"]
            assert on["resident_bilinears"] == 1 and not plans.bilinear_left and not plans["up"].emit_f32


def test_a_concat_the_plain_rule_serves_keeps_the_plain_kernel():
    """Both operands int8 on one grid and every reader at that grid: the same plan rows with the switch, no launch of the new
    entry point, nothing in requant_left."""
    from common.quantity import resident
    import concat_nets as cn
    with rd.installed():
        for make in (cn.FireNet, cn.CatReluNet, cn.FpnNet):
            net = make().eval()
            x = cn.example()
            with torch.no_grad():
                plain = net(x)
            off = resident.enable(net, x, **OFF)
            off_rows = _rows(net)
            on = resident.enable(net, x, **ON)
            assert _without(on) == off and on["requant_concats"] == 0 and _rows(net) == off_rows and not _plans(net).requant_left
            assert isinstance(net.cat.__dict__.get("forward"), resident._ConcatResident)
            _check_forwards(net, x, plain)
            assert not rd.calls


def test_the_handle_is_lossy_and_reaches_nothing_but_its_convolutions():
    from common.quantity import _native, resident
    with rd.installed():
        net = rn.DeclinedNet("ok").eval()
        x = rn.example(2, 8)
        assert resident.enable(net, x, **ON)["requant_concats"] == 1
        seen = []
        real = net.head.forward
        net.head.__dict__["forward"] = lambda t: (seen.append(t), real(t))[1]
        with torch.no_grad():
            net(x)
        del net.head.__dict__["forward"]
        h = seen[0]
        assert type(h) is resident.QHandle and h.lossy and h.exact.dtype == torch.int8 and h.grid == h.bit == 4
        assert tuple(h.shape) == (2, 32, 8, 8)
        with pytest.raises(_native.FqError, match="already quantised"):
            h.to_f32()


# ---------------------------------------------------------------- 5. what is declined
@pytest.mark.parametrize("variant", list(rn.DECLINED))
def test_what_the_plan_declines_keeps_the_off_arms_rows_and_says_why(variant):
    from common.quantity import resident
    with rd.installed():
        net = rn.DeclinedNet(variant).eval()
        x = rn.example(2, 8)
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **OFF)
        off_rows = _rows(net)
        _check_forwards(net, x, plain)
        on = resident.enable(net, x, **ON)
        plans = _plans(net)
        assert on["requant_concats"] == 0 and on["requant_sum_sources"] == 0 and _without(on) == off
        assert _rows(net) == off_rows and not isinstance(net.cat.__dict__.get("forward"), resident._ConcatRequant)
        assert list(plans.requant_left) == ["cat"] and rn.DECLINED[variant] in plans.requant_left["cat"], plans.requant_left
        _check_forwards(net, x, plain)
        assert not rd.calls


def test_a_geometry_the_kernel_does_not_take_is_declined_with_its_reason(monkeypatch):
    from common.quantity import _native, resident
    with rd.installed():
        net = rn.DeclinedNet("ok").eval()
        x = rn.example(2, 8)
        off = resident.enable(net, x, **OFF)
        off_rows = _rows(net)
        monkeypatch.setattr(_native, "concat_rq_supported", lambda *a: False)
        on = resident.enable(net, x, **ON)
        assert _without(on) == off and _rows(net) == off_rows and "unsupported geometry" in _plans(net).requant_left["cat"]


def test_a_reader_left_in_fp32_form_revokes_the_concat():
    """The walk accepts the Concat (its reader through the max-pool is a convolution at bit 4); the max-pool turns out unplanned
    (ceil_mode), so the verification takes the Concat back: the off arm's rows, and the reason names the pool."""
    from common.quantity import resident
    with rd.installed():
        net = rn.DeclinedNet("ok").eval()
        net.mp = nn.MaxPool2d(3, 1, 1, ceil_mode=True)
        head = net.head
        net.head = nn.Sequential()
        net.head.add_module("mp", net.mp)
        net.head.add_module("conv", head)
        del net.mp
        x = rn.example(2, 8)
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **OFF)
        off_rows = _rows(net)
        on = resident.enable(net, x, **ON)
        plans = _plans(net)
        assert on["requant_concats"] == 0 and _without(on) == off and _rows(net) == off_rows
        assert plans.requant_left == {"cat": "revoked by the lossy rule: read as fp32 by head.mp"}, plans.requant_left
        _check_forwards(net, x, plain)
        assert not rd.calls


# ---------------------------------------------------------------- 6. defaults, pickling, disable, flattening, run-time fallbacks
def test_the_default_call_has_no_new_key_and_plan_slots_are_unchanged():
    from common.quantity import resident
    assert resident.Plan.__slots__ == SLOTS
    with rd.installed():
        net = rn.ToyNet("two_grids").eval()
        x = rn.example()
        for kw in ({}, OFF, dict(OFF, requant=False), dict(OFF, bilinear=True, shuffle=True)):
            got = resident.enable(net, x, **kw)
            assert not NEW_KEYS & set(got) and not _plans(net).requant_left
            assert not any(isinstance(m.__dict__.get("forward"), resident._ConcatRequant) for m in net.modules())
        assert resident.enable(net, x, **OFF) == resident.enable(net, x, requant=False, **OFF)
        assert [k for k in resident.enable(net, x, **ON) if k not in NEW_KEYS] == list(resident.enable(net, x, **OFF))
        assert resident._Description.requant_left == {}
        assert not rd.calls or all(len(c) == 2 for c in rd.calls)


def test_a_planned_model_pickles_with_its_plan_and_disable_removes_it():
    from common.quantity import resident
    with rd.installed():
        net = rn.ToyNet("sum_relu").eval()
        x = rn.example()
        with torch.no_grad():
            plain = net(x)
        resident.enable(net, x, **ON)
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert _rows(again) == _rows(net) and _plans(again)["cat"].grid == (4, 5) and _plans(again)["cat"].narrow_bit == 4
        del rd.calls[:]
        _check_forwards(again, x, plain)
        assert len(rd.calls) == 3
        resident.disable(net)
        assert not _plans(net) and not _plans(net).requant_left and not any("forward" in m.__dict__ for m in net.modules())
        del rd.calls[:]
        _check_forwards(net, x, plain)
        assert not rd.calls


class _Nested(nn.Module):
    """cat1(a, b) on ONE grid (a plain Concat) inside cat2(cat1, c) with c on another grid: with flatten=True the inner one is NOT
    deferred into the re-quantising outer one, it is one int8 source of it; and cat3(cat2', d) over a re-quantising cat2' on the
    readers' bit is a plain Concat of a lossy operand."""

    def __init__(self):
        from concat_nets import conv
        super(_Nested, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.a, self.b, self.c = conv(16, 16, 1, 4, 4), conv(16, 16, 3, 4, 4, padding=1), conv(16, 16, 1, 4, 2, seed=3)
        self.d = conv(16, 16, 1, 4, 3, seed=4)
        self.cat1, self.cat2, self.cat3 = rn.Concat(), rn.Concat(), rn.Concat()
        self.head = conv(64, 8, 1, 3, 4, seed=5)

    def forward(self, x):
        s = self.r0(self.stem(x))
        return self.head(self.cat3(self.cat2(self.cat1(self.a(s), self.b(s)), self.c(s)), self.d(s)))


def test_a_requantising_concat_is_not_flattened():
    from common.quantity import resident
    with rd.installed():
        net = _Nested().eval()
        x = rn.example()
        with torch.no_grad():
            plain = net(x)
        on = resident.enable(net, x, flatten=True, **ON)
        plans = _plans(net)
        assert on["requant_concats"] == 1 and on["flattened_concats"] == 0 and on["resident_concats"] == 3, (on, plans.requant_left)
        assert type(plans["cat2"].grid) is tuple and plans["cat2"].narrow_bit == 3 and not plans["cat1"].defer and not plans["cat2"].defer
        assert plans["cat3"].grid is None and plans["cat3"].narrow_bit == 3 and not plans.requant_left
        del rd.calls[:]
        _check_forwards(net, x, plain)
        assert rd.calls == [[(32, 1, 1, False, -1), (16, 1, 1, False, 1)]] * 3
        assert on["fp32_outputs"] == 1


def test_run_time_misses_fall_back_to_the_markers_own_forward():
    from common.quantity import _native, resident
    with rd.installed():
        cat = rn.Concat()
        fwd = resident._ConcatRequant(cat)
        rng = np.random.default_rng(8)
        qa = torch.from_numpy(rng.integers(-128, 128, (2, 3, 5, 16)).astype(np.int8))
        qb = torch.from_numpy(rng.integers(-3000, 3000, (2, 3, 5, 16)).astype(np.int16))
        ha = resident.QHandle.int8(qa, 8, 4, False)
        hb = resident.QHandle.wide_narrow(12, qb, 6, None, None, True)
        ta, tb = ha.to_f32(), hb.to_f32()
        want = torch.cat([ta, tb], 1)

        def plan(**kw):
            p = resident.Plan()
            p.emit_f32, p.emit_int, p.grid, p.narrow_bit = False, True, (4, 6), 3
            for k, v in kw.items():
                setattr(p, k, v)
            cat.__dict__["_resident"] = p
            return p

        plan()
        out = fwd(ha, hb)                                     # the planned path: shifts from the HANDLES' grids
        assert type(out) is resident.QHandle and out.lossy and out.grid == out.bit == 3 and not out.relu_done and tuple(out.shape) == (2, 20, 3, 5)
        assert rd.calls == [[(8, 1, 1, False, -1), (12, 2, 1, False, -3)]]
        np.testing.assert_array_equal(out.exact.numpy(), rr.concat_rq([(qa.numpy(), 8, 1, False, -1), (qb.numpy(), 12, 1, False, -3)]))
        plan(relu=True)
        assert fwd(ha, hb).relu_done and rd.calls[-1][0][3] is True
        up = resident.DeferredUpsample(resident.QHandle.int8(torch.from_numpy(rng.integers(-128, 128, (2, 3, 5, 16)).astype(np.int8)), 8, 5, False), 2)
        big = resident.QHandle.int8(torch.from_numpy(rng.integers(-128, 128, (2, 6, 10, 16)).astype(np.int8)), 8, 4, False)
        plan()
        out = fwd(big, up)                                    # a deferred nearest upsampling is the operand's factor
        assert rd.calls[-1] == [(8, 1, 1, False, -1), (8, 1, 2, False, -2)] and up._out is None and tuple(out.shape) == (2, 16, 6, 10)
        lossy_ok = resident.QHandle.int8(qa, 8, 3, False)
        lossy_ok.lossy = True
        out = fwd(lossy_ok, hb)                               # a lossy operand at the readers' bit is copied
        assert rd.calls[-1][0] == (8, 1, 1, False, 0) and out.lossy
        del rd.calls[:]
        misses = []
        cat.__dict__.pop("_resident")
        misses.append(("no plan", fwd(ha, hb)))
        plan()
        misses.append(("fp32 tensors", fwd(ta, tb)))
        misses.append(("one fp32 tensor", fwd(ha, tb)))
        plan(grid=4)
        misses.append(("a plan of the plain kind", fwd(ha, hb)))
        plan(narrow_bit=13)
        misses.append(("a shift the kernel does not take", fwd(ha, hb)))
        plan(narrow_bit=None)
        misses.append(("no reader bit", fwd(ha, hb)))
        for what, got in misses:
            assert isinstance(got, torch.Tensor) and torch.equal(got, want), what
        plan()
        assert torch.equal(fwd(ha, ha, 2), torch.cat([ta, ta], 2))          # another dim
        assert not rd.calls
        with pytest.raises(RuntimeError):                     # planes that differ: torch.cat's own error on the fp32 forms
            fwd(ha, resident.QHandle.int8(qa[:, :2].contiguous(), 8, 4, False))
        nothing = resident.QHandle.wide_narrow(8, None, None, qa, 4, False)
        with pytest.raises(_native.FqError, match="without an exact payload"):
            fwd(nothing, hb)
        lossy = resident.QHandle.int8(qa, 8, 4, False)
        lossy.lossy = True
        with pytest.raises(_native.FqError, match="already quantised"):      # a lossy operand at another bit has no fp32 form
            fwd(lossy, hb)
        assert not rd.calls


# ---------------------------------------------------------------- 8. the random family
def _family_counts():
    kinds = [kind for seed in rn.SEEDS for _name, kind in rn.RandomRequantNet(seed).cats]
    return {k: kinds.count(k) for k in sorted(set(kinds))}, len(kinds)


def test_the_random_family_by_construction():
    """The coverage condition: over the forty models each of the three causes occurs at least ten times among the Concats the rule
    admits, and at least half of the drawn Concats are ones the plain rule does not fully serve."""
    counts, total = _family_counts()
    print("random family: %d Concats, %s" % (total, counts))
    assert set(counts) == {"reader_bit", "two_grids", "sum", "served", "declined"}
    assert all(counts[c] >= 10 for c in rn.CAUSES), counts
    assert 2 * (total - counts["served"]) >= total
    assert set(rn.RandomRequantNet(seed).plane for seed in rn.SEEDS) == {8, 16}
    assert any(st["sum_relu"] for seed in rn.SEEDS for st in rn.RandomRequantNet(seed).stages if st["kind"] == "sum")
    assert any(not st["sum_relu"] for seed in rn.SEEDS for st in rn.RandomRequantNet(seed).stages if st["kind"] == "sum")


@pytest.mark.parametrize("seed", rn.SEEDS)
def test_random_requant(seed):
    """Each drawn model under `concat`, `concat + requant` and all twelve switches: exact outputs, and with `requant` every Concat
    the rule admits by construction is planned (a condition, not a measurement), every declined one is named in requant_left and
    every served one keeps the plain kernel."""
    from common.quantity import resident
    with rd.installed_all():
        net = rn.RandomRequantNet(seed).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        want = sum(1 for _n, kind in net.cats if kind in rn.CAUSES)
        a = resident.enable(net, x, concat=True)
        assert not NEW_KEYS & set(a)
        _check_forwards(net, x, plain)
        for kw in (ON, ALL_TWELVE):
            on = resident.enable(net, x, **kw)
            plans = _plans(net)
            assert on["requant_concats"] == want, (on, net.cats, plans.requant_left)
            assert on["requant_sum_sources"] == sum(1 for _n, kind in net.cats if kind == "sum")
            for name, kind in net.cats:
                fwd = net.get_submodule(name).__dict__.get("forward")
                assert isinstance(fwd, resident._ConcatRequant) == (kind in rn.CAUSES), (name, kind)
                assert (name in plans.requant_left) == (kind == "declined"), (name, kind, plans.requant_left)
                if kind in rn.CAUSES:
                    assert not plans[name].emit_f32 and plans[name].emit_int
                if kind == "served":
                    assert isinstance(fwd, resident._ConcatResident) and not plans[name].emit_f32
            _check_forwards(net, x, plain)
        resident.disable(net)
        _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 9. the mixed family with the twelfth switch
@pytest.mark.parametrize("index", [i for i, _seed in mn.family()][:8])
def test_random_mixed_nets_with_all_twelve_switches(index, oracle):
    from common.quantity import resident
    seed = dict(mn.family())[index]
    with rd.installed_all():
        _info, (net,) = mn.calibrated(index, seed, [rd.installed_all])
        x, x2 = mn.inputs(net, index, seed)
        with torch.no_grad():
            want = [net(x).clone(), net(x2).clone()]
        eleven = resident.enable(net, x, **{k: v for k, v in ALL_TWELVE.items() if k != "requant"})
        twelve = resident.enable(net, x, **ALL_TWELVE)
        assert set(twelve) == set(eleven) | NEW_KEYS
        print("mixed %d: requant_concats %d, left %s" % (index, twelve["requant_concats"], _plans(net).requant_left))
        with torch.no_grad():
            assert torch.equal(net(x), want[0]) and torch.equal(net(x2), want[1])
        resident.disable(net)
        with torch.no_grad():
            assert torch.equal(net(x), want[0])


# ---------------------------------------------------------------- 10. the model file
def test_resunet_plans_every_concat_over_its_stage_sums():
    """ResUNet, base width 8, one block per stage, every layer at bit 4 (no calibration): each Concat joins the int16 sum of a
    stage -- the first at an unaligned channel offset of the launch -- with a bilinear upsampling; without requant every one of them
    and every upsampling leaves the integer domain."""
    from common.quantity import resident
    import depthwise_nets as dn
    m = rn.resunet_model(num_classes=3, input_size=32, base_width=8, layers=(1, 1, 1, 1), batch_norm=False).eval()
    x = rn.example(2, 32)
    with rd.installed():
        gen = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * ((2.0 / max(1, p[0].numel())) ** 0.5 if p.dim() > 1 else 0.05))
        net = dn.rebuild(m, dn.fixed_info(m, out_bits=(4,), image_bit=5))
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, concat=True, bilinear=True)
        off_plans = _plans(net)
        on = resident.enable(net, x, concat=True, bilinear=True, requant=True)
        plans = _plans(net)
        assert on["requant_concats"] == 3 and on["requant_sum_sources"] == 3 and on["resident_bilinears"] == 3, (on, plans.requant_left, plans.bilinear_left)
        assert off["resident_bilinears"] == 0 and off["resident_concats"] == 0 and len(off_plans.bilinear_left) == 3
        assert on["fp32_outputs"] == 1 and off["fp32_outputs"] > 6 and not plans.requant_left and not plans.bilinear_left
        del rd.calls[:]
        _check_forwards(net, x, plain)
        assert [[(c, by) for c, by, _up, _relu, _shift in call] for call in rd.calls[:3]] == [[(32, 2), (64, 1)], [(16, 2), (32, 1)], [(8, 2), (16, 1)]]
        for stage in ("layer1", "layer2", "layer3"):
            p = plans[stage + ".0.Eltwise"]
            assert p.want_wide and p.relu and not p.emit_f32 and off_plans[stage + ".0.Eltwise"].emit_f32, stage


# ---------------------------------------------------------------- 11. golden G26: a calibrated net with a residual skip
@pytest.fixture(scope="module")
def g26(golden_dir):
    with open(os.path.join(golden_dir, "g26_requant_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g26_requant_net.npz"))


def test_g26_meets_the_makers_conditions(g26):
    """On the reference's own run: a Concat whose reader sits on another bit than one of its operands, one with operands on two
    grids, one with an Eltwise operand (here the same Concat); the golden holds the recipe and recorded outputs only."""
    ref, arrays = g26
    info, q = ref["net_info"], ref["quantity_information"]
    assert all(ref["conditions"][k] for k in ("reader_bit_differs", "two_grids", "eltwise_operand"))
    cats = [k for k in ref["net_info_order"] if info[k]["type"] == "Concat"]
    assert len(cats) == 2 and [info[i]["type"] for i in info[cats[0]]["inputs"]] == ["Eltwise", "Conv2d"]
    assert q["conv5"]["output_bit"] != q["conv6"]["input_bit"] or q["conv3"]["output_bit"] != q["conv6"]["input_bit"]
    assert ref["seed"] == rn.G26_SEED and set(arrays.files) == {"x", "logits_recon"}


def test_g26_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g26, oracle):
    """The reference's graph discovery, merge groups, feat.table, weight.table and quantity information of requant_nets.g26_net byte
    for byte through the oracle-backed CPU engine on the SHIPPED settings, and its ReconModel logits bit for bit: plain, with
    concat + bilinear and with requant=True on top."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g26
    shape = rn.G26_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(an.integer_weights(rn.g26_net(), base_seed=rn.G26_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(an.integer_batches(3, shape, rn.G26_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(an.integer_weights(rn.g26_net(), base_seed=rn.G26_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with rd.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = an.integer_input(shape, rn.G26_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x, concat=True, bilinear=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off_plans = _plans(net)
                assert not rd.calls
                on = resident.enable(net, x, concat=True, bilinear=True, requant=True)
                del rd.calls[:]
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            plans = _plans(net)
            print("G26: off %s\n on %s\n left %s / %s; launches %s" % (off, on, plans.bilinear_left, plans.requant_left, rd.calls))
            assert on["requant_concats"] >= 1 and on["requant_sum_sources"] == 1 and not plans.requant_left, (on, plans.requant_left)
            assert type(plans["Concat1"].grid) is tuple and plans["Concat1"].narrow_bit == info["conv6"]["input_bit"]
            # (the sum on its own grid, max(0, conv3's, conv1's); the upsampling's lossy value on the readers' bit already)
            assert plans["Concat1"].grid == (max(0, info["conv3"]["output_bit"], info["conv1"]["output_bit"]), plans["Concat1"].narrow_bit)
            assert plans["up1"].grid == info["conv5"]["output_bit"] != plans["up1"].narrow_bit and rd.calls[0][0][1] == 2
            # (the max-pool behind the skip still reads the sum as fp32 -- a max-pool over a sum is left out --; the Concat reads its integers)
            assert not off_plans["Eltwise1"].emit_int and plans["Eltwise1"].emit_int and plans["Eltwise1"].want_wide
            assert on["resident_bilinears"] == 1 and off["resident_bilinears"] == 0 and on["fp32_outputs"] < off["fp32_outputs"]
