"""The resident add with a nearest-upsampled operand (fq_add_up_resident, csrc/fq_add_up.hip) against the rule of include/fq.h:
int_conv_ref.add_resident_ref -- fq_add_resident's expression in NumPy -- on the np.repeat-ed coarse operand.  Everything is
integers: every comparison is exact.   pytest -m gpu"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import int_conv_ref
import topdown_nets as tn

pytestmark = pytest.mark.gpu

FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = 0, -1, -4
SENTINEL, GUARD = 0x5A, 64
DTYPES = ((np.int8, np.int8), (np.int8, np.int16), (np.int16, np.int8), (np.int16, np.int16))
OUTPUTS = ((True, True), (True, False), (False, True))       # (wide, narrow)
GRID_PAIRS = list(itertools.product(tn.GRIDS, tn.GRIDS))


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _ptr(t):
    return None if t is None else (ctypes.c_void_p(t) if isinstance(t, int) else ctypes.c_void_p(t.data_ptr()))


def _raw(nat, x, xb, gx, y, yb, gy, up, wide, g_wide, narrow, ib, relu, N, H, W, cpad):
    return nat.lib().fq_add_up_resident(_ptr(x), xb, gx, _ptr(y), yb, gy, up, _ptr(wide), g_wide, _ptr(narrow), ib, relu, N, H, W,
                                        cpad, None)


def _guarded(shape, dtype):
    """(buffer, view): the output as a 16-byte aligned view with GUARD sentinel bytes in front of and behind it."""
    size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
    view = buf[GUARD:GUARD + size].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all())


def _run(nat, x, gx, y, gy, up, want_wide, want_narrow, ib, relu):
    """One launch into guarded views -> (wide or None, narrow or None) as NumPy arrays."""
    g = max(0, gx, gy)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    wb, wv = _guarded(x.shape, torch.int16) if want_wide else (None, None)
    nb, nv = _guarded(x.shape, torch.int8) if want_narrow else (None, None)
    N, H, W, cpad = x.shape
    rc = _raw(nat, xd, x.itemsize, gx, yd, y.itemsize, gy, up, wv, g, nv, ib, int(relu), N, H, W, cpad)
    assert rc == FQ_OK, rc
    torch.cuda.synchronize()
    assert all(_guards_intact(b) for b in (wb, nb) if b is not None)
    np.testing.assert_array_equal(xd.cpu().numpy(), x)                          # the operands are only read
    np.testing.assert_array_equal(yd.cpu().numpy(), y)
    return (wv.cpu().numpy() if want_wide else None), (nv.cpu().numpy() if want_narrow else None)


def _reference(x, gx, y_big, gy, g, ib, relu):
    """int_conv_ref.add_resident_ref.  Its own assert refuses |wide| = 32768, although the sum -128 on grid 8 IS the int16
    -32768 (no ReLU, both operands at their negative ends -- which the sources plant).  Those elements are taken out of the call
    (operands zeroed) and held against the closed form instead: s = -128, wide = -128 * 2^8, narrow = clamp(rint(-128 * 2^ib))."""
    low = np.zeros(x.shape, bool)
    if g == 8 and not relu:
        low = x.astype(np.float64) * 2.0 ** -gx + y_big.astype(np.float64) * 2.0 ** -gy <= -128.0
    wide, narrow = int_conv_ref.add_resident_ref(np.where(low, 0, x), gx, np.where(low, 0, y_big), gy, g, ib, relu)
    wide[low] = -32768
    narrow[low] = np.int8(np.clip(np.rint(-128.0 * 2.0 ** ib), -128, 127))
    return wide, narrow


# ---------------------------------------------------------------- 1. the kernel against the rule
@pytest.mark.parametrize("case", tn.KERNEL_CASES, ids=tn.case_arg)
def test_add_up_kernel_vs_the_rule(nat, case):
    """All four operand widths and all sixteen grid pairs per shape; g - ib, the ReLU and the outputs rotate, so that over the
    case list every grid pair meets every k and the packed (k in 1 .. 8 with small shifts), int32 and fp32 forms all run."""
    N, H, W, C, up = case
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    turn = tn.KERNEL_CASES.index(case)
    for (xt, yt) in DTYPES:
        for (gx, gy) in GRID_PAIRS:
            turn += 1
            g = max(0, gx, gy)
            k = tn.K_VALUES[turn % len(tn.K_VALUES)]
            relu = bool((turn // 5) % 2)
            want_wide, want_narrow = OUTPUTS[(turn // 3) % 3]
            x = tn.source(rng, (N, H, W, tn.pad16(C)), C, xt, gx)
            y = tn.source(rng, (N, H // up, W // up, tn.pad16(C)), C, yt, gy)
            assert x.min() == (-128 if xt == np.int8 else -128 << max(gx, 0)) and x.max() == (127 if xt == np.int8 else 127 << max(gx, 0))
            wide, narrow = _run(nat, x, gx, y, gy, up, want_wide, want_narrow, g - k, relu)
            ref_wide, ref_narrow = _reference(x, gx, tn.repeat(y, up), gy, g, g - k, relu)
            what = str((xt.__name__, yt.__name__, gx, gy, k, relu, want_wide, want_narrow))
            if want_wide:
                np.testing.assert_array_equal(wide, ref_wide, err_msg=what)
            if want_narrow:
                np.testing.assert_array_equal(narrow, ref_narrow, err_msg=what)


def test_the_rotation_covers_what_it_claims():
    """(host arithmetic) over the case list every (dtype pair, k, ReLU, outputs) combination and every (grid pair, k) occurs."""
    seen, grids = set(), set()
    for i, _case in enumerate(tn.KERNEL_CASES):
        turn = i
        for d in range(4):
            for pair in GRID_PAIRS:
                turn += 1
                seen.add((d, tn.K_VALUES[turn % 5], bool((turn // 5) % 2), OUTPUTS[(turn // 3) % 3]))
                grids.add((pair, tn.K_VALUES[turn % 5]))
    assert len(seen) == 4 * 5 * 2 * 3 and len(grids) == 16 * 5
    assert {c[3] for c in tn.KERNEL_CASES} == {1, 16, 19, 100} and {c[4] for c in tn.KERNEL_CASES} == {2, 4}
    assert {c[0] for c in tn.KERNEL_CASES} == {1, 3} and {c[1:3] for c in tn.KERNEL_CASES if c[4] == 4} == {(4, 4), (4, 12), (8, 8)}


def test_narrow_only_above_grid_8(nat):
    """g = max(gx, gy) > 8: the exact sum does not fit int16, so `wide` is FQ_ERR_UNSUPPORTED with nothing written; the
    re-quantisation alone is taken (the fp32 form)."""
    rng = np.random.default_rng(9)
    for (xt, yt) in DTYPES:
        for (gx, gy, ib) in ((10, 3, 4), (2, 9, 9), (12, 12, 6)):
            x = tn.source(rng, (3, 4, 12, 32), 19, xt, min(gx, 8))
            y = tn.source(rng, (3, 2, 6, 32), 19, yt, min(gy, 8))
            _wide, narrow = _run(nat, x, gx, y, gy, 2, False, True, ib, True)
            s = np.clip(x.astype(np.float64) * 2.0 ** -gx + tn.repeat(y, 2).astype(np.float64) * 2.0 ** -gy, 0.0, 127.0)
            np.testing.assert_array_equal(narrow, np.clip(np.rint(s * 2.0 ** ib), -128, 127).astype(np.int8))
            xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            wb, wv = _guarded(x.shape, torch.int16)
            assert _raw(nat, xd, x.itemsize, gx, yd, y.itemsize, gy, 2, wv, max(gx, gy), None, ib, 1, 3, 4, 12, 32) == FQ_ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert bool((wb == SENTINEL).all())


def test_a_lane_takes_a_second_item(nat):
    """tn.SECOND_ITEM_CASE, derived from csrc/fq_add_up_geom.h: 1 051 392 items on 4096 x 256 lanes, so the first 2 816 lanes
    take a second item through the digit-wise walk (three items per pixel: the walk carries)."""
    N, H, W, C, up = tn.SECOND_ITEM_CASE
    items = N * H * W * tn.pad16(C) // 16
    assert items > tn.LANES >= N * (H - up) * (W - up) * tn.pad16(C) // 16
    rng = np.random.default_rng(5)
    for (xt, yt) in ((np.int8, np.int16), (np.int16, np.int8)):
        x = tn.source(rng, (N, H, W, tn.pad16(C)), C, xt, 4)
        y = tn.source(rng, (N, H // up, W // up, tn.pad16(C)), C, yt, 3)
        wide, narrow = nat.add_up_resident(torch.from_numpy(x).cuda(), 4, torch.from_numpy(y).cuda(), 3, up, True, 4, True, 2, False)
        ref_wide, ref_narrow = _reference(x, 4, tn.repeat(y, up), 3, 4, 2, False)
        np.testing.assert_array_equal(wide.cpu().numpy(), ref_wide)
        np.testing.assert_array_equal(narrow.cpu().numpy(), ref_narrow)


# ---------------------------------------------------------------- 2. what the entry point declines
def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any geometry that could be launched, and nothing may be launched."""
    x = torch.ones(2, 8, 8, 32, dtype=torch.int16, device="cuda")
    y = torch.ones(2, 4, 4, 32, dtype=torch.int16, device="cuda")
    wide = torch.full((2, 8, 8, 32), 5, dtype=torch.int16, device="cuda")
    narrow = torch.full((2, 8, 8, 32), 5, dtype=torch.int8, device="cuda")
    sup = nat.lib().fq_add_up_resident_supported
    bad, un = FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED

    def call(x=x, xb=1, gx=4, y=y, yb=1, gy=4, up=2, wide=wide, g_wide=4, narrow=narrow, ib=4, relu=0, N=2, H=8, W=8, cpad=32):
        return _raw(nat, x, xb, gx, y, yb, gy, up, wide, g_wide, narrow, ib, relu, N, H, W, cpad)

    assert call(x=None) == bad and call(y=None) == bad and call(wide=None, narrow=None) == bad            # null operands, no output
    for name, t in (("x", x), ("y", y), ("wide", wide), ("narrow", narrow)):                              # misaligned pointers
        assert call(**{name: t.data_ptr() + 8}) == bad, name
    assert call(xb=0) == bad and call(xb=4) == bad and call(yb=3) == bad                                   # element sizes
    assert call(cpad=24) == bad and call(cpad=-16) == bad and call(N=-1) == bad and call(H=-2) == bad and call(W=-8) == bad
    assert call(H=7) == bad and call(W=6, up=4) == bad and call(H=6, W=6, up=4) == bad                    # planes the factor does not divide
    assert call(gx=17) == bad and call(gy=-17) == bad and call(ib=17) == bad                               # grids and bits outside [-16, 16]
    assert call(up=1) == un and call(up=3) == un and call(up=8) == un and call(up=0) == un and call(up=-2) == un
    assert call(g_wide=3) == un and call(gx=9, g_wide=9) == un                                             # fq_add_resident's own
    assert sup(2, 8, 8, 32) == 1 and sup(4, 8, 8, 32) == 1 and sup(4, 4, 12, 112) == 1
    assert sup(3, 9, 9, 32) == 0 and sup(2, 7, 8, 32) == 0 and sup(4, 8, 6, 32) == 0 and sup(2, 8, 8, 24) == 0 and sup(2, 0, 8, 32) == 0
    for empty in (dict(N=0), dict(H=0), dict(W=0), dict(cpad=0)):                                          # empty tensors
        assert call(x=None, y=None, wide=None, narrow=None, **empty) == FQ_OK, empty
    torch.cuda.synchronize()
    assert bool((wide == 5).all()) and bool((narrow == 5).all())                                           # nothing was launched
    assert call(xb=2, yb=2) == FQ_OK
    torch.cuda.synchronize()
    assert bool((wide == 2 << 0).all()) and bool((narrow == 2).all())                                      # 1 * 2^-4 + 1 * 2^-4 on grid 4 and at bit 4
    # the Python wrapper: wrong dtypes, devices and shapes raise, nothing is launched
    with pytest.raises(nat.FqError):
        nat.add_up_resident(x.float(), 4, y, 4, 2, True, 4, True, 4, False)
    with pytest.raises(nat.FqError):
        nat.add_up_resident(x.cpu(), 4, y.cpu(), 4, 2, True, 4, True, 4, False)
    with pytest.raises(nat.FqError):
        nat.add_up_resident(x, 4, y, 4, 4, True, 4, True, 4, False)
    with pytest.raises(nat.FqError):
        nat.add_up_resident(x, 4, x, 4, 2, True, 4, True, 4, False)
    assert nat.add_up_supported(2, 8, 8, 32) and not nat.add_up_supported(3, 9, 9, 32)
