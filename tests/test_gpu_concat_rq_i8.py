"""The re-quantising concatenation (fq_concat_rq_i8_nhwc, csrc/fq_concat_i8.hip) against the closed form in NumPy
(tests/requant_ref.py, which test_requant_plan_cpu.py holds against the reference's literal chain).  Everything is integers: every
comparison is exact.   pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import requant_nets as rn
import requant_ref as rr

pytestmark = pytest.mark.gpu

FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = 0, -1, -4
SENTINEL, GUARD = 0x5A, 64


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _run(nat, case, rng):
    N, H, W, Cs, ups, by, shifts, relus = case
    arrays = rn.sources(rng, case)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    want = rr.concat_rq([(a, C, up, relu, shift) for a, C, up, relu, shift in zip(arrays, Cs, ups, relus, shifts)])
    total = sum(Cs)
    assert want.shape == (N, H, W, rn.pad16(total))
    srcs = [(d, C, up, relu, shift) for d, C, up, relu, shift in zip(dev, Cs, ups, relus, shifts)]
    # the output is a view inside a larger buffer: sentinel bytes in front of and behind it must survive
    buf = torch.full((GUARD + want.size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
    view = buf[GUARD:GUARD + want.size].view(want.shape)
    assert view.data_ptr() % 16 == 0
    got = nat.concat_rq_i8_nhwc(srcs, out=view)
    assert got is view
    head, body, tail = buf[:GUARD].cpu().numpy(), view.cpu().numpy(), buf[GUARD + want.size:].cpu().numpy()
    assert np.array_equal(body, want), (case, np.argwhere(body != want)[:4])
    assert (head == SENTINEL).all() and (tail == SENTINEL).all()
    assert not body[..., total:].any()                                      # the padding channels are zero, whatever the sources' hold
    for a, d in zip(arrays, dev):
        assert np.array_equal(d.cpu().numpy(), a)                           # the sources are only read
    return srcs, want


# ---------------------------------------------------------------- 1. the kernel against the closed form
@pytest.mark.parametrize("plane", rn.KERNEL_PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("nsrc", rn.KERNEL_NSRC)
def test_concat_rq_kernel_vs_closed_form(nat, nsrc, plane):
    """Every channel list of the source count with every int8 / int16 mix on this plane, N 1 and 3: chunks that hold bytes of
    several sources, int16 sources at unaligned channel offsets, factors 1, 2 and 4, shifts -8 .. 8, a ReLU flag per source; the
    extremes of both types and exact ties planted, garbage in the sources' padding channels, sentinels around the output."""
    rng = np.random.default_rng(1000 * nsrc + 10 * plane[0] + plane[1])
    cases = rn.kernel_cases(nsrc, plane)
    assert set(s for c in cases for s in c[6]) <= set(rn.KERNEL_SHIFTS) and len(cases) >= 10
    last = None
    for case in cases:
        last = _run(nat, case, rng)
    srcs, want = last
    own = nat.concat_rq_i8_nhwc(srcs)                                       # ... and the allocating form
    assert tuple(own.shape) == want.shape and np.array_equal(own.cpu().numpy(), want)


def test_a_launch_large_enough_that_lanes_take_a_second_item(nat):
    case = rn.BIG_CASE
    assert case[0] * case[1] * case[2] * (rn.pad16(sum(case[3])) // 16) > 2048 * 256
    _run(nat, case, np.random.default_rng(5))
    aligned = (4, 96, 96, (64, 128, 64), (1, 2, 1), (2, 1, 1), (-2, 3, 0), (1, 0, 0))      # the aligned family, strided too
    assert aligned[0] * aligned[1] * aligned[2] * 16 > 2048 * 256
    _run(nat, aligned, np.random.default_rng(6))


# (N, H, W, Cs, ups, ReLU flags): the aligned family with an upsampled source; byte-shifted parts and chunks that straddle; one
# source and the tail mask
IDENTITY_CASES = ((2, 4, 4, (16, 32), (1, 2), (0, 1)), (2, 4, 4, (1, 3, 16, 19), (1, 1, 2, 1), (0, 1, 0, 1)), (2, 4, 4, (5,), (1,), (1,)))


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=lambda c: "C" + "_".join(map(str, c[3])))
def test_int8_sources_at_shift_0_give_the_bytes_of_the_moving_kernel(nat, case):
    """Both entry points are one kernel skeleton with two element policies: with every source int8 and every shift 0 the
    re-quantisation is the identity, and the output is fq_concat_n_i8_nhwc's on the same sources, factors and ReLU flags, byte
    for byte."""
    N, H, W, Cs, ups, relus = case
    zeros = (0,) * len(Cs)
    arrays = rn.sources(np.random.default_rng(sum(Cs)), (N, H, W, Cs, ups, (1,) * len(Cs), zeros, relus))
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    moved = nat.concat_n_i8_nhwc([(d, C, up, relu) for d, C, up, relu in zip(dev, Cs, ups, relus)])
    requantised = nat.concat_rq_i8_nhwc([(d, C, up, relu, 0) for d, C, up, relu in zip(dev, Cs, ups, relus)])
    assert moved.shape == requantised.shape == (N, H, W, rn.pad16(sum(Cs))) and torch.equal(moved, requantised)


# ---------------------------------------------------------------- 2. what the entry point declines
def _raw(nat, srcs, nsrc, out, cpad_out, N, H, W):
    arr = (nat._CatSrcRq * max(len(srcs), 1))()
    for i, (q, by, C, cpad, up, relu, shift) in enumerate(srcs):
        ptr = q if isinstance(q, int) or q is None else q.data_ptr()
        arr[i].q, arr[i].bytes, arr[i].C, arr[i].Cpad, arr[i].up, arr[i].relu, arr[i].shift = ptr, by, C, cpad, up, relu, shift
    optr = out if isinstance(out, int) or out is None else out.data_ptr()
    return nat.lib().fq_concat_rq_i8_nhwc(arr, nsrc, ctypes.c_void_p(optr) if optr is not None else None, cpad_out, N, H, W, None)


def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any of these geometries that could launch, and nothing may be
    launched.  The size guards are met with these small buffers and oversized dimensions: no giant allocation."""
    a = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    b = torch.zeros(1, 8, 8, 32, dtype=torch.int16, device="cuda")
    c = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    out = torch.full((1, 8, 8, 160), 5, dtype=torch.int8, device="cuda")
    A, B, C = (a, 1, 16, 16, 1, 0, -3), (b, 2, 16, 16, 1, 1, 2), (c, 1, 16, 16, 1, 0, 0)
    ok3 = [A, B, C]
    INV, UNS = FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED
    assert _raw(nat, ok3, 0, out, 48, 1, 4, 4) == INV and _raw(nat, ok3, -1, out, 48, 1, 4, 4) == INV               # nsrc < 1
    assert nat.lib().fq_concat_rq_i8_nhwc(None, 3, ctypes.c_void_p(out.data_ptr()), 48, 1, 4, 4, None) == INV
    assert _raw(nat, [A] * 9, 9, out, 144, 1, 4, 4) == UNS                                             # nsrc > 8
    assert _raw(nat, ok3, 3, None, 48, 1, 4, 4) == INV                                                 # no output
    assert _raw(nat, ok3, 3, out.data_ptr() + 8, 48, 1, 4, 4) == INV                                   # misaligned output
    assert _raw(nat, [A, (None, 2, 16, 16, 1, 0, 0), C], 3, out, 48, 1, 4, 4) == INV                   # no source
    assert _raw(nat, [A, B, (c.data_ptr() + 4, 1, 16, 16, 1, 0, 0)], 3, out, 48, 1, 4, 4) == INV       # misaligned source
    assert _raw(nat, [A, (b, 2, 0, 16, 1, 0, 0), C], 3, out, 32, 1, 4, 4) == INV                       # C < 1
    assert _raw(nat, [A, (b, 2, 16, 16, 0, 0, 0), C], 3, out, 48, 1, 4, 4) == INV                      # up < 1
    assert _raw(nat, [A, (b, 2, 16, 8, 1, 0, 0), C], 3, out, 48, 1, 4, 4) == INV                       # Cpad < C
    assert _raw(nat, [A, (b, 2, 16, 16, 1, 2, 0), C], 3, out, 48, 1, 4, 4) == INV                      # relu outside {0, 1}
    for by in (0, 3, 4, -1):
        assert _raw(nat, [A, (b, by, 16, 16, 1, 0, 0), C], 3, out, 48, 1, 4, 4) == INV, by             # bytes outside {1, 2}
    assert _raw(nat, ok3, 3, out, 64, 1, 4, 4) == INV                                                  # wrong Cpad_out
    assert _raw(nat, [(a, 1, 16, 16, 1, 0, 0)], 1, out, 16, 1, 4, 4) == INV                            # nothing to do
    for sh in (9, -9, 100):
        assert _raw(nat, [A, (b, 2, 16, 16, 1, 0, sh), C], 3, out, 48, 1, 4, 4) == UNS, sh             # |shift| > 8
    assert _raw(nat, [A, (b, 2, 16, 16, 3, 0, 0), C], 3, out, 48, 1, 6, 6) == UNS                      # another factor
    assert _raw(nat, [A, (b, 2, 16, 16, 2, 0, 0), C], 3, out, 48, 1, 7, 8) == UNS                      # H % up != 0
    assert _raw(nat, [A, B, (c, 1, 16, 16, 4, 0, 0)], 3, out, 48, 1, 8, 6) == UNS                      # W % up != 0
    assert _raw(nat, [A, (b, 2, 16, 24, 1, 0, 0), C], 3, out, 48, 1, 4, 4) == UNS                      # Cpad % 16 != 0
    assert _raw(nat, [(a, 1, 30000, 30000, 1, 0, 1), (b, 2, 30000, 30000, 1, 0, 0), (c, 1, 5537, 5552, 1, 0, 0)], 3, out, 65552, 1, 1, 1) == UNS
    assert _raw(nat, ok3, 3, out, 48, 1 << 12, 1 << 10, 1 << 10) == UNS                                # 2^31 - 1 bytes or more of output
    assert _raw(nat, [A, (b, 2, 16, 1 << 19, 1, 0, 0), C], 3, out, 48, 1, 64, 32) == UNS               # ... an int16 source (2^31 bytes exactly)
    assert _raw(nat, [(None, 1, 16, 16, 1, 0, 0)] * 3, 3, None, 48, 0, 4, 4) == FQ_OK                  # N == 0: no launch, no pointer read
    torch.cuda.synchronize()
    assert bool((out == 5).all())                                   # nothing was launched
    o48 = torch.full((1, 8, 8, 48), 5, dtype=torch.int8, device="cuda")
    assert _raw(nat, ok3, 3, o48, 48, 1, 8, 8) == FQ_OK
    o16 = torch.full((1, 8, 8, 16), 5, dtype=torch.int8, device="cuda")
    assert _raw(nat, [(b, 2, 16, 32, 1, 0, 0)], 1, o16, 16, 1, 8, 8) == FQ_OK                          # an int16 source at shift 0 is work
    assert _raw(nat, [(a, 1, 16, 32, 1, 0, 1)], 1, o16, 16, 1, 8, 8) == FQ_OK                          # ... and so is a shift alone
    torch.cuda.synchronize()
    assert not bool(o48.any()) and not bool(o16.any())
    with pytest.raises(nat.FqError, match="different output planes"):
        nat.concat_rq_i8_nhwc([(a, 16, 1, False, 0), (b[:, :4].contiguous(), 16, 1, False, 1)])
    with pytest.raises(nat.FqError, match="no operand"):
        nat.concat_rq_i8_nhwc([])
    with pytest.raises(nat.FqError, match="not int8 or int16"):
        nat.concat_rq_i8_nhwc([(a.to(torch.int32), 16, 1, False, 1)])
    L = nat.lib()
    ci3 = ctypes.c_int * 3
    assert L.fq_concat_rq_i8_nhwc_supported(ci3(16, 1, 30), ci3(1, 2, 4), ci3(1, 2, 1), ci3(-8, 0, 8), 3) == 1
    assert L.fq_concat_rq_i8_nhwc_supported(ci3(16, 1, 30), ci3(1, 2, 4), ci3(1, 2, 1), ci3(-9, 0, 8), 3) == 0
    assert L.fq_concat_rq_i8_nhwc_supported(ci3(16, 1, 30), ci3(1, 2, 4), ci3(1, 3, 1), ci3(0, 0, 0), 3) == 0
