"""resident.enable(..., concat=True, bilinear=True) on a box without a GPU: nn.Upsample(scale_factor=2 or 4,
mode="bilinear", align_corners=False) between an int8 activation and the convolutions behind it as ONE integer function.  The
closed form (tests/bilinear_ref.py) against the reference's chain taken literally (tests/bilinear_doubles.py: the oracle's
DeQuantity -> torch's F.interpolate -> ReLU -> the oracle's Quantity); the tracer, the plan, the handles and the module glue run
for real on oracle-backed doubles; every declined reason with its text; the host arithmetic of fq_upsample_bilinear_i8_nhwc; the
kernel's index arithmetic walked on the host (scripts/upsample_bilinear_geom_check.cpp); golden G25 pins a calibrated toy U-Net to
the reference; forty random U-Net-shaped nets run under three plans.  Every comparison is exact."""
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
import bilinear_doubles as bd
import bilinear_nets as bn
import bilinear_ref as br
import mixed_nets as mn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, HIP, UNSUPPORTED = -1, -2, -4
OFF = dict(concat=True, shuffle=True)
ON = dict(concat=True, shuffle=True, bilinear=True)
ALL_ELEVEN = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
                  sums=True, topdown=True, bilinear=True)
SLOTS = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg", "fuse_next",
         "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip", "perm", "table")


def _plans(model):
    from common.quantity import resident
    return resident.describe(model)


def _rows(model):
    def plain(v):
        return tuple(v.tolist()) if isinstance(v, torch.Tensor) else v       # (a table activation's 256 entries)
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


# ---------------------------------------------------------------- 1. the closed form against the literal chain
def _planes(rng, h, w):
    """random planes, +-extremes alternating, constant -128: int8 [3, h, w, 4]"""
    x = rng.integers(-128, 128, (3, h, w, 4)).astype(np.int8)
    x[1] = np.where((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0, -128, 127)[:, :, None]
    x[2, :, :, :2] = -128
    return x


@pytest.mark.parametrize("up", (2, 4))
def test_the_closed_form_is_the_literal_chain_on_all_256_constant_planes_and_every_shift(up, oracle):
    """Every constant plane (256 values as channels of one 3 x 2 plane), every shift in [-8, 8], grids -2, 0, 3, 8, ReLU on and
    off: S = D^2 q there, so this walks the rounding -- ties included -- over every integer a constant region can hold."""
    x = np.broadcast_to(np.arange(-128, 128).astype(np.int8)[None, None, None, :], (1, 3, 2, 256)).copy()
    for g in bn.CLOSED_FORM_GRIDS:
        for shift in range(-8, 9):
            for relu in (False, True):
                want = bd.literal_chain(x, 256, up, g, g + shift, relu)
                got = br.upsample(x, 256, up, shift, relu)
                np.testing.assert_array_equal(got, want, err_msg=str((g, shift, relu)))


@pytest.mark.parametrize("up", (2, 4))
def test_the_closed_form_is_the_literal_chain_on_random_and_extreme_planes(up, oracle):
    rng = np.random.default_rng(30 + up)
    ties = 0
    for (h, w) in bn.CLOSED_FORM_PLANES:
        x = _planes(rng, h, w)
        S = br.sums(x, up)
        assert np.abs(S).max() <= 128 * (2 * up) ** 2
        for g in bn.CLOSED_FORM_GRIDS:
            for shift in range(-8, 9):
                for relu in (False, True):
                    want = bd.literal_chain(x, 4, up, g, g + shift, relu)
                    np.testing.assert_array_equal(br.requant(S, up, shift, relu), want, err_msg=str((h, w, g, shift, relu)))
                k = 2 * int(np.log2(2 * up)) - shift
                if k > 0:
                    ties += int(((S & ((1 << k) - 1)) == (1 << (k - 1))).sum())
    assert ties > 100                                         # (the half-to-even branch is walked, both ways)


def test_the_double_zeroes_the_padding_and_depends_on_the_shift_alone(oracle):
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(-128, 128, (2, 3, 5, 32)).astype(np.int8))
    y = bd.upsample_bilinear_i8_nhwc(x, 19, 2, 1, True)
    assert tuple(y.shape) == (2, 6, 10, 32) and not y[..., 19:].any() and int(y.min()) == 0
    np.testing.assert_array_equal(y.numpy(), br.upsample(x.numpy(), 19, 2, 1, True))
    for g in (-2, 3, 8):                                      # (what the double relies on: every step scales by a power of two)
        np.testing.assert_array_equal(bd.literal_chain(x.numpy(), 19, 2, g, g + 1, True), y.numpy()[..., :19])


# ---------------------------------------------------------------- 2. the switch, the entry points, the settings
def test_bilinear_needs_concat():
    from common.quantity import resident
    with bd.installed():
        net = bn.DecoderNet().eval()
        for kw in (dict(bilinear=True), dict(bilinear=True, concat=False), dict(bilinear=True, shuffle=True, activations=True)):
            with pytest.raises(ValueError, match="concat=True"):
                resident.enable(net, bn.example(), **kw)
        assert not resident.is_enabled(net)


def test_the_binding_and_the_header_symbol_exist():
    from common.quantity import _native
    assert callable(_native.upsample_bilinear_i8_nhwc) and callable(_native.upsample_bilinear_supported)
    with open(os.path.join(ROOT, "include", "fq.h")) as fh:
        text = fh.read()
    assert re.search(r"^int fq_upsample_bilinear_i8_nhwc\(const int8_t\* x, int8_t\* y, int N, int H, int W, int C, int Cpad,", text, re.M)
    assert re.search(r"^int fq_upsample_bilinear_i8_nhwc_supported\(int up, int shift", text, re.M)
    assert "rounded half to even" in text and "ONE integer rounding and no fp32 step" in text
    L = _native.lib()
    assert L.fq_upsample_bilinear_i8_nhwc.restype is ctypes.c_int and len(L.fq_upsample_bilinear_i8_nhwc.argtypes) == 11


def test_upsample_is_in_both_lists_of_the_shipped_settings():
    import yaml
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    assert "Upsample" in settings["ALL_OP_TYPE"] and "Upsample" in settings["ALLOW_SAME_TID_OP_TYPE"]
    assert "Upsample" not in settings["CARE_OP_TYPE"] and "Upsample" not in settings["MERGE_OP_YTPE"]
    for lst in ("ALL_OP_TYPE", "ALLOW_SAME_TID_OP_TYPE", "CARE_OP_TYPE"):
        assert "UpsamplingBilinear2d" not in settings[lst]      # (the align_corners=True form)
    assert type(bn.bilinear(2)).__name__ == "Upsample"


def test_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.upsample_bilinear_supported
    for up in range(-1, 10):
        for shift in range(-12, 13):
            assert ok(up, shift) == (up in (2, 4) and abs(shift) <= 8), (up, shift)


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
def test_the_host_side_guards_and_their_return_codes(L, buf):
    p, p2, raw = buf
    fn = L.fq_upsample_bilinear_i8_nhwc
    good = (p, p2, 1, 2, 2, 10, 16, 2, 0, 0)                 # (x, y, N, H, W, C, Cpad, up, shift, relu)

    def with_(**kw):
        names = ("x", "y", "N", "H", "W", "C", "Cpad", "up", "shift", "relu")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    invalid = {"null x": with_(x=None), "null y": with_(y=None), "misaligned x": with_(x=ctypes.c_void_p(p.value + 4)),
               "misaligned y": with_(y=ctypes.c_void_p(p2.value + 8)), "N < 0": with_(N=-1), "H = 0": with_(H=0), "W < 0": with_(W=-3),
               "C = 0": with_(C=0), "C > Cpad": with_(C=17), "Cpad % 16": with_(Cpad=24, C=20), "Cpad = 0": with_(Cpad=0),
               "y inside x": with_(y=ctypes.c_void_p(p.value + 32)), "x inside y": with_(x=ctypes.c_void_p(p2.value + 64))}
    for what, a in invalid.items():
        assert fn(*a, None) == INVALID, what
    unsupported = {"up 3": with_(up=3), "up 1": with_(up=1), "up 8": with_(up=8), "up 0": with_(up=0), "shift 9": with_(shift=9),
                   "shift -9": with_(shift=-9), "2^31 - 1 bytes out": with_(N=1, H=1, W=(1 << 31) // 64, Cpad=16, C=16),
                   "far over": with_(N=1 << 16, H=1 << 16, W=1 << 16), "up 4 over": with_(up=4, H=4096, W=2048)}
    for what, a in unsupported.items():
        assert fn(*a, None) == UNSUPPORTED, what
    # an invalid argument is named before an unsupported one; N == 0 is fine whatever the pointers are
    assert fn(*with_(C=0, up=3), None) == INVALID
    assert fn(*with_(N=0, x=None, y=None), None) == 0 and fn(*with_(N=0), None) == 0
    assert fn(*with_(N=0, up=3), None) == UNSUPPORTED
    # what passes the guards is launched: with no GPU the launch fails, and that -- not a refusal -- is what comes back
    for a in (good, with_(up=4, shift=8, relu=1), with_(shift=-8), with_(H=1, W=1, C=1)):
        assert fn(*a, None) == HIP, a
    assert raw.raw == b"\x55" * (4096 + 64)
    # just under the limit: 2^31 - 2 bytes or fewer of output pass the guard (pointers that are never touched: the launch fails first)
    big = ctypes.c_void_p(1 << 44)
    assert fn(p, big, 1, 4096, 8191, 16, 16, 2, 0, 0, None) == HIP
    assert fn(p, big, 1, 4096, 8192, 16, 16, 2, 0, 0, None) == UNSUPPORTED


# ---------------------------------------------------------------- 3. the walker
def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_upsample_bilinear_i8_geom.h holds the kernel's lane -> (item, taps, weights, offsets) functions and its rounding, and
    compiles as host code: scripts/upsample_bilinear_geom_check.cpp, built with the address and undefined-behaviour sanitizers,
    walks every lane of every launch and exits non-zero on a load outside the source, an unaligned access, taps or weights that
    are not the closed form, an output element written zero times or twice, or a rounding that is not half to even."""
    exe = str(tmp_path / "upsample_bilinear_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "upsample_bilinear_geom_check.cpp")])
    shapes = ["%d,%d,%d,%d,%d" % (n, p[0], p[1], c, up) for up in (2, 4) for n in (1, 3) for p in bn.KERNEL_PLANES + (bn.BIG_PLANE,)
              for c in bn.KERNEL_CHANNELS]
    shapes.append("1,592,592,48,2")                          # past 4096 x 256 lanes: a second item per lane
    out = subprocess.run([exe] + shapes, capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(shapes) + 1 and not out.stderr, out.stdout[-2000:] + out.stderr
    words = lines[-2].split()
    items = 592 * 592 * 3
    assert int(words[words.index("items") + 1]) == items > 4096 * 256 and int(words[words.index("blocks") + 1]) == 4096
    assert int(words[words.index("second-items") + 1]) == items - 4096 * 256
    big = [ln for ln in lines if ln.startswith("case 1,33,47,")]
    assert len(big) == 2 * len(bn.KERNEL_CHANNELS) and all(int(ln.split()[ln.split().index("blocks") + 1]) > 1 for ln in big)
    for bad in ("1,4,4,16,3", "1,0,4,16,2", "1,4,4,0,2"):
        assert subprocess.run([exe, bad], capture_output=True, text=True).returncode == 1
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_upsample_bilinear_i8_geom.h")).read()
    assert re.search(r"kUpbBlock = 256;", header) and re.search(r"kUpbMaxBlocks = 256 \* 16;", header)
    assert re.search(r"kUpbMaxBytes = 0x7ffffffeL;", header) and re.search(r"kUpbMaxShift = 8;", header)


# ---------------------------------------------------------------- 4. what is planned
@pytest.mark.parametrize("variant", bn.DECODER_VARIANTS)
def test_the_two_level_decoder(variant):
    """Each upsampling is one launch of the new entry point, the convolution in front of it goes from emit_f32 to integers only,
    the Concat behind it is planned, and on == off == plain on the example, on one image and on a flipped batch."""
    from common.quantity import resident
    with bd.installed():
        net = bn.DecoderNet(variant).eval()
        x = bn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **OFF)
        off_plans = _plans(net)
        _check_forwards(net, x, plain)
        assert "resident_bilinears" not in off and not bd.calls and not off_plans.bilinear_left
        assert all(off_plans[f].emit_f32 for f in net.front) and not any(u in off_plans for u in net.ups)
        on = resident.enable(net, x, **ON)
        plans = _plans(net)
        assert set(on) == set(off) | {"resident_bilinears"} and on["resident_bilinears"] == len(net.ups) and not plans.bilinear_left
        del bd.calls[:]
        _check_forwards(net, x, plain)
        assert len(bd.calls) == 3 * len(net.ups)
        for f, u in zip(net.front, net.ups):
            p = plans[u]
            assert plans[f].emit_int and not plans[f].emit_f32, (f, plans[f])
            assert p.emit_int and not p.emit_f32 and p.up == (4 if variant == "x4" else 2) and p.table is None and not p.defer
            assert isinstance(net.get_submodule(u).__dict__.get("forward"), resident._BilinearResident)
            assert p.grid == net.get_submodule(f).output_bit and p.narrow_bit == 4
        assert plans["up1"].relu == (variant == "relu")
        if variant == "relu":
            assert isinstance(net.r_up.__dict__.get("forward"), resident._ReluPassThrough)
            assert bd.calls[0][4] is True and int(plans["up1"].relu) == 1
        if variant == "shift":
            assert (plans["up1"].grid, plans["up1"].narrow_bit) == (2, 4) and bd.calls[0][3] == 2
        assert bd.calls[0][:3] == (24, (4, 4, 4, 32), 4 if variant == "x4" else 2)
        want_cats = {"x4": 1, "conv": 1}.get(variant, 2)
        assert on["resident_concats"] == want_cats and off["resident_concats"] == 0
        assert on["fp32_outputs"] == 1 and off["fp32_outputs"] == 1 + want_cats + len(net.ups)        # (the head alone leaves as fp32)
        if variant == "pool":
            assert not plans["mp"].emit_f32
        if variant == "slice":
            assert not plans["cut"].emit_f32 and bd.calls[0][0] == 24


def test_the_handle_is_lossy_and_reaches_nothing_but_its_convolutions():
    from common.quantity import _native, resident
    with bd.installed():
        net = bn.DeclinedNet("ok").eval()
        x = bn.example(2, 8)
        resident.enable(net, x, concat=True, bilinear=True)
        seen = []
        real = net.head.forward
        net.head.__dict__["forward"] = lambda t: (seen.append(t), real(t))[1]
        with torch.no_grad():
            net(x)
        del net.head.__dict__["forward"]
        h = seen[0]
        assert type(h) is resident.QHandle and h.lossy and h.exact.dtype == torch.int8 and h.grid == h.bit == 4
        assert tuple(h.shape) == (2, 16, 16, 16)
        with pytest.raises(_native.FqError, match="already quantised"):
            h.to_f32()


# ---------------------------------------------------------------- 5. what is declined
@pytest.mark.parametrize("variant", list(bn.DECLINED))
def test_what_the_plan_declines_keeps_the_off_arms_rows_and_says_why(variant):
    from common.quantity import resident
    with bd.installed():
        net = bn.DeclinedNet(variant).eval()
        x = bn.example(2, 8)
        kw = dict(concat=True, activations=variant in ("lossy", "act"))
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **kw)
        off_rows = _rows(net)
        _check_forwards(net, x, plain)
        on = resident.enable(net, x, bilinear=True, **kw)
        plans = _plans(net)
        assert on["resident_bilinears"] == 0 and {k: v for k, v in on.items() if k != "resident_bilinears"} == off
        assert _rows(net) == off_rows and "up" not in plans and "forward" not in net.up.__dict__
        assert list(plans.bilinear_left) == ["up"] and bn.DECLINED[variant] in plans.bilinear_left["up"], plans.bilinear_left
        assert plans["mid"].emit_f32 or variant in ("lossy", "no_source", "fp32_source", "sum")
        _check_forwards(net, x, plain)
        assert not bd.calls


def test_a_table_activation_in_front_of_a_bilinear_is_left_with_the_walks_reason():
    from common.quantity import resident
    with bd.installed():
        net = bn.DeclinedNet("lossy").eval()
        x = bn.example(2, 8)
        on = resident.enable(net, x, concat=True, activations=True, bilinear=True)
        plans = _plans(net)
        assert on["resident_activations"] == 0 and on["resident_bilinears"] == 0
        assert "read as fp32 by the bilinear upsampling up" in plans.activations_left["act"]
        assert "bilinear" not in resident._MOVES and "upsample" in resident._MOVES


def test_a_concat_on_another_grid_revokes_the_upsampling():
    """The skip of the first Concat on grid 3, its reader at bit 4: the walk accepts up1 (its only convolution reads at bit 4), the
    Concat cannot be planned (operands on two grids), and the verification takes the upsampling back."""
    from common.quantity import resident
    with bd.installed():
        net = bn.DecoderNet("plain").eval()
        net.enc.output_bit = 3
        x = bn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **OFF)
        off_rows = _rows(net)
        on = resident.enable(net, x, **ON)
        plans = _plans(net)
        assert on["resident_bilinears"] == 1 and list(plans.bilinear_left) == ["up1"]
        assert plans.bilinear_left["up1"] == "revoked by the lossy rule: read as fp32 by cat1"
        rows = _rows(net)
        for name in ("mid", "bott", "enc", "pool1", "pool2"):   # (the first level is the off arm's; the second one is planned)
            assert rows[name] == off_rows[name], name
        assert plans["mid"].emit_f32 and not plans["dec1"].emit_f32 and "forward" not in net.up1.__dict__
        assert off["resident_concats"] == 0 and on["resident_concats"] == 1
        _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 6. defaults, pickling, disable, run-time fallbacks
def test_the_default_call_has_no_new_key_and_plan_slots_are_unchanged():
    from common.quantity import resident
    assert resident.Plan.__slots__ == SLOTS
    with bd.installed():
        net = bn.DecoderNet().eval()
        x = bn.example()
        for kw in ({}, dict(concat=True), OFF, dict(OFF, bilinear=False)):
            got = resident.enable(net, x, **kw)
            assert "resident_bilinears" not in got and not _plans(net).bilinear_left
            assert not any(isinstance(m.__dict__.get("forward"), resident._BilinearResident) for m in net.modules())
        assert resident.enable(net, x, **OFF) == resident.enable(net, x, bilinear=False, **OFF)
        assert list(resident.enable(net, x, **ON))[:9] == list(resident.enable(net, x, **OFF))[:9]
        assert resident._Description.bilinear_left == {}


def test_a_planned_model_pickles_with_its_plan_and_disable_removes_it():
    from common.quantity import resident
    with bd.installed():
        net = bn.DecoderNet("relu").eval()
        x = bn.example()
        with torch.no_grad():
            plain = net(x)
        resident.enable(net, x, **ON)
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert _rows(again) == _rows(net) and _plans(again)["up1"].up == 2 and _plans(again)["up1"].relu
        del bd.calls[:]
        _check_forwards(again, x, plain)
        assert len(bd.calls) == 6
        resident.disable(net)
        assert not _plans(net) and not _plans(net).bilinear_left and not any("forward" in m.__dict__ for m in net.modules())
        del bd.calls[:]
        _check_forwards(net, x, plain)
        assert not bd.calls


def test_run_time_misses_fall_back_to_the_modules_own_forward():
    from common.quantity import _native, resident
    with bd.installed():
        up = bn.bilinear(2)
        fwd = resident._BilinearResident(up)
        rng = np.random.default_rng(8)
        q = torch.from_numpy(rng.integers(-128, 128, (2, 3, 5, 16)).astype(np.int8))
        h = resident.QHandle.int8(q, 8, 4, False)
        t = h.to_f32()
        want = nn.functional.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)

        def plan(**kw):
            p = resident.Plan()
            p.emit_f32, p.emit_int, p.up, p.grid, p.narrow_bit = False, True, 2, 4, 4
            for k, v in kw.items():
                setattr(p, k, v)
            up.__dict__["_resident"] = p
            return p

        plan()
        out = fwd(h)                                          # the planned path
        assert type(out) is resident.QHandle and out.lossy and len(bd.calls) == 1 and out.grid == 4 and not out.relu_done
        np.testing.assert_array_equal(out.exact.numpy(), br.upsample(q.numpy(), 8, 2, 0, False))
        plan(relu=True)
        assert fwd(h).relu_done and bd.calls[-1][4] is True
        del bd.calls[:]
        misses = []
        up.__dict__.pop("_resident")
        misses.append(("no plan", fwd(h)))
        plan()
        misses.append(("an fp32 tensor", fwd(t)))
        wide = resident.QHandle.wide_narrow(8, q.to(torch.int16), 4, None, None, False)
        misses.append(("an int16 payload", fwd(wide)))
        plan(grid=3)
        misses.append(("another grid", fwd(h)))
        plan(narrow_bit=13)
        misses.append(("a shift the kernel does not take", fwd(h)))
        plan(up=4)
        misses.append(("another factor than the module's", fwd(h)))
        plan()
        lossy = resident.QHandle.int8(q, 8, 4, False)
        lossy.lossy = True
        carried = resident.carry(t.clone(), lossy)
        misses.append(("a lossy source carried by an fp32 tensor", fwd(carried)))
        for what, got in misses:
            assert isinstance(got, torch.Tensor) and torch.equal(got, want), what
        assert not bd.calls
        with pytest.raises(_native.FqError, match="already quantised"):      # a lossy handle has no fp32 form to fall back to
            fwd(lossy)


# ---------------------------------------------------------------- 7. golden G25: a calibrated toy U-Net
@pytest.fixture(scope="module")
def g25(golden_dir):
    with open(os.path.join(golden_dir, "g25_bilinear_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g25_bilinear_net.npz"))


def test_g25_upsamplings_are_pruned_and_read_at_one_bit(g25):
    ref, _arrays = g25
    info, q = ref["net_info"], ref["quantity_information"]
    assert not any(v["type"] in ("Upsample", "MaxPool2d", "ReLU") for v in info.values())
    convs = [None] + [k for k in ref["net_info_order"] if info[k]["type"] == "Conv2d"]
    cats = [None] + [k for k in ref["net_info_order"] if info[k]["type"] == "Concat"]
    assert sorted(info[cats[1]]["inputs"]) == sorted([convs[2], convs[4]]) and sorted(info[cats[2]]["inputs"]) == sorted([convs[1], convs[5]])
    assert info[convs[8]]["inputs"] == [convs[7]]
    assert q["conv5"]["input_bit"] == q["Concat1"]["output_bit"] == q["conv2"]["output_bit"] == q["conv4"]["output_bit"]
    assert q["conv6"]["input_bit"] == q["Concat2"]["output_bit"] == q["conv1"]["output_bit"] == q["conv5"]["output_bit"]
    assert q["conv8"]["input_bit"] == q["conv7"]["output_bit"]


def test_g25_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g25, oracle):
    """The reference's graph discovery, merge groups, feat.table, weight.table and quantity information of bilinear_nets.g25_net
    byte for byte through the oracle-backed CPU engine on the SHIPPED settings, and its ReconModel logits bit for bit: plain, with
    concat=True and with concat=True, bilinear=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g25
    shape = bn.G25_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(an.integer_weights(bn.g25_net(), base_seed=bn.G25_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(an.integer_batches(3, shape, bn.G25_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(an.integer_weights(bn.g25_net(), base_seed=bn.G25_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with bd.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = an.integer_input(shape, bn.G25_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x, concat=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off_plans = _plans(net)
                assert not bd.calls
                on = resident.enable(net, x, concat=True, bilinear=True)
                del bd.calls[:]
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            plans = _plans(net)
            assert on["resident_bilinears"] == 3 and not plans.bilinear_left, (on, plans.bilinear_left)
            assert [c[2] for c in bd.calls] == [2, 2, 4, 2, 2, 4] and [c[4] for c in bd.calls[:3]] == [True, False, False]
            assert on["resident_concats"] == 2 and off["resident_concats"] == 0
            for front, up in (("conv4", "up1"), ("conv5", "up2"), ("conv7", "up3")):
                assert off_plans[front].emit_f32 and not plans[front].emit_f32 and not plans[up].emit_f32, front
                assert plans[up].grid == info[front]["output_bit"]
            assert plans["up1"].relu and plans["up1"].narrow_bit == info["conv5"]["input_bit"]
            assert plans["up3"].up == 4 and plans["up3"].narrow_bit == info["conv8"]["input_bit"]


# ---------------------------------------------------------------- 8. the random family
FAMILY_COUNTS = (74, 62)    # (bilinear upsamplings of the forty models, those the rule admits by construction)


def test_the_random_family_by_construction():
    ups = [u for seed in bn.SEEDS for u in bn.RandomBilinearNet(seed).ups]
    assert all(len(bn.RandomBilinearNet(seed).ups) >= 1 for seed in bn.SEEDS)
    got = (len(ups), sum(1 for _n, ok in ups if ok))
    print("random family: %d bilinear upsamplings, %d admitted" % got)
    assert got == FAMILY_COUNTS and 2 * got[1] >= got[0]
    assert set(f for seed in bn.SEEDS for f in bn.RandomBilinearNet(seed).factors) == {2, 4}
    assert set(len(bn.RandomBilinearNet(seed).factors) for seed in bn.SEEDS) == {1, 2, 3}
    assert set(bn.RandomBilinearNet(seed).plane for seed in bn.SEEDS) == {8, 16}



@pytest.mark.parametrize("seed", bn.SEEDS)
def test_random_bilinear(seed):
    """Each drawn model under `concat`, `concat + bilinear` and all eleven switches: exact outputs, and with `bilinear` every
    upsampling the rule admits is planned (a condition, not a measurement), every other one is named in bilinear_left."""
    from common.quantity import resident
    with bd.installed_all():
        net = bn.RandomBilinearNet(seed).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        want = sum(1 for _n, ok in net.ups if ok)
        a = resident.enable(net, x, concat=True)
        assert "resident_bilinears" not in a
        _check_forwards(net, x, plain)
        for kw in (dict(concat=True, bilinear=True), ALL_ELEVEN):
            on = resident.enable(net, x, **kw)
            plans = _plans(net)
            assert on["resident_bilinears"] == want, (on, net.ups, plans.bilinear_left)
            for name, ok in net.ups:
                assert (name in plans.bilinear_left) == (not ok), (name, plans.bilinear_left)
                assert (name in plans and isinstance(net.get_submodule(name).__dict__.get("forward"), resident._BilinearResident)) == ok, name
            _check_forwards(net, x, plain)
        resident.disable(net)
        _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 9. the mixed family with the eleventh switch
@pytest.mark.parametrize("index", [i for i, _seed in mn.family()][:8])
def test_random_mixed_nets_with_all_eleven_switches(index, oracle):
    from common.quantity import resident
    seed = dict(mn.family())[index]
    with bd.installed_all():
        _info, (net,) = mn.calibrated(index, seed, [bd.installed_all])
        x, x2 = mn.inputs(net, index, seed)
        with torch.no_grad():
            want = [net(x).clone(), net(x2).clone()]
        ten = resident.enable(net, x, **{k: v for k, v in ALL_ELEVEN.items() if k != "bilinear"})
        ten_rows = _rows(net)
        eleven = resident.enable(net, x, **ALL_ELEVEN)
        assert set(eleven) == set(ten) | {"resident_bilinears"} and eleven["resident_bilinears"] == 0      # (the family has no bilinear module)
        assert _rows(net) == ten_rows
        with torch.no_grad():
            assert torch.equal(net(x), want[0]) and torch.equal(net(x2), want[1])
        resident.disable(net)
        with torch.no_grad():
            assert torch.equal(net(x), want[0])


# ---------------------------------------------------------------- 10. the model file
def test_unet_needs_a_multiple_of_two_to_the_depth_and_plans_its_decoder():
    from common.quantity import resident
    import depthwise_nets as dn
    for size, depth in ((0, 2), (12, 3), (31, 1), (225, 4), (8, 4)):
        with pytest.raises(ValueError):
            bn.unet_model(input_size=size, depth=depth)
    m = bn.unet_model(num_classes=3, input_size=16, base_width=8, depth=2, batch_norm=False).eval()
    ups = [mod for mod in m.modules() if isinstance(mod, nn.Upsample)]
    assert len(ups) == 2 and all(u.mode == "bilinear" and not u.align_corners and u.scale_factor == 2 for u in ups)
    assert sum(type(mod).__name__ == "Concat" for mod in m.modules()) == 2 and sum(isinstance(mod, nn.MaxPool2d) for mod in m.modules()) == 2
    x = bn.example(2, 16)
    with torch.no_grad():
        assert tuple(m(x).shape) == (2, 3, 16, 16)
    assert tuple(bn.unet_model(input_size=32, base_width=4, depth=4).eval()(bn.example(1, 32)).shape) == (1, 2, 32, 32)
    with bd.installed():
        gen = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * ((2.0 / max(1, p[0].numel())) ** 0.5 if p.dim() > 1 else 0.05))
        net = dn.rebuild(m, dn.fixed_info(m, out_bits=(4,), image_bit=5))
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, concat=True)
        on = resident.enable(net, x, concat=True, bilinear=True)
        assert on["resident_bilinears"] == 2 and on["resident_concats"] == 2 and off["resident_concats"] == 0
        assert on["fp32_outputs"] == 1 and off["fp32_outputs"] == 5 and not _plans(net).bilinear_left
        _check_forwards(net, x, plain)
