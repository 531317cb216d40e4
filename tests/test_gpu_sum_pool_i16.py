"""Windowed average pooling over the exact int16 sum of a resident NewAdd (fq_avgpool_i16_nhwc, csrc/fq_avgpool_i16.hip) against
the rule of include/fq.h in NumPy float32 (avgpool_nets.numpy_rule, which tests/test_sum_pool_plan_cpu.py holds against torch's own
chain on int16 sources).  Everything is integers: every comparison is exact.   pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import avgpool_nets as an
import sum_pool_nets as sn

pytestmark = pytest.mark.gpu

FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = 0, -1, -4
SENTINEL, GUARD = 0x5A, 64


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------- 1. the kernel against the rule
def _run_in_view(nat, x_dev, want, C, kernel, stride, padding, cip, shift, relu):
    """The output is a view inside a larger buffer: sentinel bytes in front of and behind it must survive."""
    buf = torch.full((GUARD + want.size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
    view = buf[GUARD:GUARD + want.size].view(want.shape)
    assert view.data_ptr() % 16 == 0
    got = nat.avgpool_i16_nhwc(x_dev, C, kernel, stride, padding, cip, shift, relu, out=view)
    assert got is view
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + want.size:] == SENTINEL).all()
    return host[GUARD:GUARD + want.size].reshape(want.shape)


# (kind, grid): all of int16; what a sum on the coarsest, a middle and the finest grid holds at its two ends
SOURCES = (("random", 0), ("max", 0), ("min", 0), ("max", 3), ("min", 3), ("max", 8), ("min", 8), ("grid", 8))


@pytest.mark.parametrize("case", an.KERNEL_CASES, ids=an.case_arg)
def test_avgpool_i16_kernel_vs_the_rule(nat, case):
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    C, kernel, stride, padding = case[3], case[4:6], case[6:8], case[8:10]
    for kind, g in SOURCES:
        x = sn.source16(rng, case, kind, g)
        assert x.dtype == np.int16 and (x[..., C:].all() or C == x.shape[-1])       # garbage in the source's padding channels
        if kind == "random":
            assert x.min() == -32768 and x.max() == 32767
        x_dev = torch.from_numpy(x).cuda()
        for cip in (False, True):
            for relu in (False, True):
                for shift in an.SHIFTS:
                    want = an.numpy_rule(x, C, kernel, stride, padding, cip, shift, relu)
                    got = _run_in_view(nat, x_dev, want, C, kernel, stride, padding, cip, shift, relu)
                    np.testing.assert_array_equal(got, want, err_msg=str((kind, g, cip, relu, shift)))
                    assert not got[..., C:].any()                               # zeros in the output's
        np.testing.assert_array_equal(x_dev.cpu().numpy(), x)                   # the source is only read
    own = nat.avgpool_i16_nhwc(x_dev, C, kernel, stride, padding, True, -8, False)          # ... and the allocating form
    assert tuple(own.shape) == (case[0],) + an.out_plane(case) + (an.pad16(C),) and own.dtype == torch.int8
    np.testing.assert_array_equal(own.cpu().numpy(), an.numpy_rule(x, C, kernel, stride, padding, True, -8, False))


def test_the_sources_cover_what_they_claim():
    cs = an.KERNEL_CASES
    assert {c[3] for c in cs} == {1, 16, 19, 100} and set(an.SHIFTS) == {-8, -1, 0, 1, 8}
    # |S| reaches 64 * 32768 at the cap; the ends of a grid-8 sum saturate at shift 0 and survive at shift -8
    cap = (1, 16, 8, 19, 8, 8, 8, 8, 0, 0)
    lo = sn.source16(None, cap, "min", 8)
    assert int(lo[..., :19].astype(np.int64).reshape(2, 8, 8, 19).sum(axis=(1, 2)).min()) == -64 * 32768
    assert (an.numpy_rule(lo, 19, (8, 8), (8, 8), (0, 0), True, 0, False)[..., :19] == -128).all()
    assert (an.numpy_rule(lo, 19, (8, 8), (8, 8), (0, 0), True, -8, False)[..., :19] == -128).all()
    hi = sn.source16(None, cap, "max", 8)
    assert (an.numpy_rule(hi, 19, (8, 8), (8, 8), (0, 0), True, -8, False)[..., :19] == 127).all()
    assert (an.numpy_rule(hi, 19, (8, 8), (8, 8), (0, 0), True, -1, True)[..., :19] == 127).all()


@pytest.mark.parametrize("g", sn.GRIDS)
def test_ties_round_half_to_even(nat, g):
    """tie_source scaled by 2^g: the window means are k + 0.5 on the pool's output grid at shift -g, and at shift -g - 1."""
    x = sn.tie_source16(g)
    x_dev = torch.from_numpy(x).cuda()
    for shift, want in ((-g, [[0, 2, 2], [0, -2, -2], [1, 3, -1]]), (-g - 1, [[0, 1, 1], [0, -1, -1], [0, 2, 0]])):
        if shift < -8:
            continue
        rule = an.numpy_rule(x, 16, (2, 2), (2, 2), (0, 0), True, shift, False)
        assert rule[0, :, :, 0].tolist() == want                                # half away from zero would give 1, 2, 3, -1, ...
        got = nat.avgpool_i16_nhwc(x_dev, 16, (2, 2), (2, 2), (0, 0), True, shift, False).cpu().numpy()
        np.testing.assert_array_equal(got, rule)


def test_more_items_than_lanes(nat):
    """532 512 items of 8 channels on 2048 x 256 lanes: the first 8 224 lanes take a second item."""
    case = sn.STRIDE_LOOP_CASE
    assert case[0] * case[1] * case[2] * (case[3] // 8) > 2048 * 256 >= case[0] * (case[1] - 1) * (case[2] - 1) * (case[3] // 8)
    x = sn.source16(np.random.default_rng(5), case)
    got = nat.avgpool_i16_nhwc(torch.from_numpy(x).cuda(), case[3], (3, 3), (1, 1), (1, 1), False, -7, True).cpu().numpy()
    np.testing.assert_array_equal(got, an.numpy_rule(x, case[3], (3, 3), (1, 1), (1, 1), False, -7, True))


# ---------------------------------------------------------------- 2. what the entry point declines
def _raw(nat, x, y, N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, cip=1, shift=0, relu=0):
    ptr = lambda t: None if t is None else (ctypes.c_void_p(t) if isinstance(t, int) else ctypes.c_void_p(t.data_ptr()))
    return nat.lib().fq_avgpool_i16_nhwc(ptr(x), ptr(y), N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, cip, shift, relu, None)


def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any geometry that could be launched, and nothing may be launched."""
    x = torch.ones(2, 16, 16, 32, dtype=torch.int16, device="cuda")
    y = torch.full((2, 16, 16, 32), 5, dtype=torch.int8, device="cuda")
    sup = nat.lib().fq_avgpool_i16_nhwc_supported
    ok = (2, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1)
    bad = FQ_ERR_INVALID_ARG
    assert _raw(nat, None, y, *ok) == bad and _raw(nat, x, None, *ok) == bad                             # null pointers
    assert _raw(nat, x.data_ptr() + 4, y, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 1) == bad                       # misaligned source
    assert _raw(nat, x, y.data_ptr() + 8, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 1) == bad                       # misaligned output
    assert _raw(nat, x, y, -1, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1) == bad                                   # sizes
    assert _raw(nat, x, y, 2, 0, 16, 20, 32, 3, 3, 1, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 0, 20, 32, 3, 3, 1, 1, 1, 1) == bad
    assert _raw(nat, x, y, 2, 16, 16, 0, 32, 3, 3, 1, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 0, 3, 3, 1, 1, 1, 1) == bad
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 0, 3, 1, 1, 0, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 0, 1, 1, 1, 0) == bad    # kernel
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 0, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, -1, 1, 1) == bad   # stride
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, -1, 1) == bad                                   # negative padding
    assert _raw(nat, x, y, 2, 16, 16, 33, 32, 3, 3, 1, 1, 1, 1) == bad                                    # C > Cpad
    assert _raw(nat, x, y, 2, 16, 16, 20, 24, 3, 3, 1, 1, 1, 1) == bad                                    # Cpad % 16
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, 2, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, 1, 2) == bad    # 2 pad > kernel
    assert _raw(nat, x, y, 2, 4, 16, 20, 32, 7, 3, 2, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 4, 20, 32, 3, 7, 1, 2, 1, 1) == bad      # P < 1, Q < 1
    un = FQ_ERR_UNSUPPORTED
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 9, 9, 1, 1, 4, 4) == un and sup(9, 9, 1, 1, 4, 4, 0) == 0   # 81 taps
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 5, 13, 1, 1, 0, 0) == un and sup(5, 13, 1, 1, 0, 0, 0) == 0  # 65 taps
    assert _raw(nat, x, y, *ok, shift=9) == un and _raw(nat, x, y, *ok, shift=-9) == un
    assert sup(3, 3, 1, 1, 1, 1, 9) == 0 and sup(3, 3, 1, 1, 1, 1, -9) == 0
    assert _raw(nat, x, y, 1, 32768, 32768, 16, 16, 2, 2, 2, 2, 0, 0) == un                               # a source of 2^35 bytes
    assert _raw(nat, x, y, 1, 32768, 2048, 16, 16, 2, 2, 2, 2, 0, 0) == un                                # ... of 2^31 bytes (2^30 elements)
    assert _raw(nat, x, y, 1, 32768, 4096, 8, 16, 1, 1, 1, 1, 0, 0) == un                                 # (an output of 2^31 bytes behind a source of 2^32)
    assert _raw(nat, x, y, 2147483647, 2147483647, 2147483647, 16, 2147483632, 1, 1, 1, 1, 0, 0) == un    # products past 2^63
    assert sup(3, 3, 1, 1, 1, 1, 0) == 1 and sup(8, 8, 8, 8, 4, 4, 8) == 1 and sup(2, 3, 1, 2, 1, 1, -8) == 1
    assert sup(3, 3, 1, 1, 2, 1, 0) == 0 and sup(0, 3, 1, 1, 0, 0, 0) == 0 and sup(3, 3, 0, 1, 0, 0, 0) == 0 and sup(3, 3, 1, 1, -1, 0, 0) == 0
    assert _raw(nat, None, None, 0, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1) == FQ_OK                            # N == 0
    torch.cuda.synchronize()
    assert bool((y == 5).all())                                                                           # nothing was launched
    assert _raw(nat, x, y, *ok) == FQ_OK
    torch.cuda.synchronize()
    assert not bool((y == 5).any())
    # the Python wrapper: wrong dtypes and a window that does not fit raise, nothing is launched
    with pytest.raises(nat.FqError):
        nat.avgpool_i16_nhwc(x.to(torch.int8), 20, (3, 3), (1, 1), (1, 1), True, 0, False)
    with pytest.raises(nat.FqError):
        nat.avgpool_i16_nhwc(x.cpu(), 20, (3, 3), (1, 1), (1, 1), True, 0, False)
    with pytest.raises(nat.FqError):
        nat.avgpool_i16_nhwc(x, 20, (19, 3), (1, 1), (1, 1), True, 0, False)
    with pytest.raises(nat.FqError):
        nat.avgpool_i16_nhwc(x, 20, (3, 3), (1, 1), (1, 1), True, 9, False)
