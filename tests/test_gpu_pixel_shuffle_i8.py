"""fq_pixel_shuffle_i8_nhwc on the MI355X against torch's CPU pixel_shuffle / pixel_unshuffle on the same integers
(pixelshuffle_nets.torch_rule), and against the index rule in numpy.  Every comparison is exact.   pytest -m gpu

The shapes (pixelshuffle_nets.kernel_cases) are the smallest at which each mechanism can go wrong: one pixel, planes that are no
square, more than one workgroup; C below 4, no multiple of 4, one below, at and one above 16, multiples of 16 (the register
transpose for r = 2 and 4) and 100; every factor, both directions; one and three images.  Every case asserts which kernel family
it selected.  The source's padding channels hold random garbage, the output is pre-filled with 0x55 and lies inside a larger
allocation whose bytes in front of and behind it must stay as they were.  Two launches have more items than the capped grid has
lanes, one per family, so that the stride loop iterates."""
import ctypes

import numpy as np
import pytest
import torch

import pixelshuffle_nets as pn

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, UNSUPPORTED = -1, -4


def _run(case, seed):
    from common.quantity import _native
    N, H, W, C, r, inverse = case
    x = pn.source(np.random.default_rng(seed), case)
    want = pn.torch_rule(x, C, r, inverse)
    assert _native.pixel_shuffle_supported(C, r, inverse) and _native.pixel_shuffle_family(C, r, inverse) == pn.family(C, r)
    nbytes = want.size
    arena = torch.full((GUARD + nbytes + GUARD,), 0x55, dtype=torch.int8, device="cuda")
    out = arena[GUARD:GUARD + nbytes].view(want.shape)
    xd = torch.from_numpy(x).cuda()
    got = _native.pixel_shuffle_i8_nhwc(xd, C, r, inverse, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = arena.cpu().numpy()
    assert (host[:GUARD] == 0x55).all() and (host[GUARD + nbytes:] == 0x55).all(), case
    np.testing.assert_array_equal(host[GUARD:GUARD + nbytes].reshape(want.shape), want, err_msg=str(case))
    np.testing.assert_array_equal(xd.cpu().numpy(), x)                                  # the source is only read
    return x, want, xd


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("r", pn.FACTORS)
def test_kernel_matches_torch_and_writes_nothing_outside_its_output(r, inverse):
    from common.quantity import _native
    families = set()
    for k, case in enumerate(pn.kernel_cases(r, inverse)):
        x, want, xd = _run(case, seed=1000 * r + 100 * inverse + k)
        C = case[3]
        real = C * r * r if inverse else C
        assert not want[..., real:].any()
        families.add(_native.pixel_shuffle_family(C, r, inverse))
        if k % 10 == 0:                                                                 # the index rule, and a fresh output tensor
            np.testing.assert_array_equal(pn.pixel_rule(x, C, r, inverse), want)
            np.testing.assert_array_equal(_native.pixel_shuffle_i8_nhwc(xd, C, r, inverse).cpu().numpy(), want)
    assert families == ({pn.GENERAL} if r == 3 else {pn.ALIGNED, pn.GENERAL})          # both families are hit


@pytest.mark.parametrize("case", pn.BIG_CASES, ids=pn.case_arg)
def test_a_launch_whose_lanes_take_a_second_item(case):
    N, H, W, C, r, inverse = case
    items = N * H * W * (C // 16) if pn.family(C, r) == pn.ALIGNED else N * H * W * pn.pad16(C * r * r) // 16
    assert items > pn.BLOCK * pn.MAX_BLOCKS
    _run(case, seed=7)


def test_unshuffle_of_shuffle_is_the_identity_on_the_device():
    from common.quantity import _native
    for C, r in ((16, 2), (32, 4), (5, 3), (3, 2)):
        x = torch.from_numpy(pn.source(np.random.default_rng(C), (2, 5, 4, C, r, 0))).cuda()
        back = _native.pixel_shuffle_i8_nhwc(_native.pixel_shuffle_i8_nhwc(x, C, r, 0), C, r, 1)
        assert torch.equal(back[..., :C * r * r], x[..., :C * r * r]) and not back[..., C * r * r:].any()


def test_every_refusal_by_return_code_with_nothing_written():
    from common.quantity import _native
    L = _native.lib()
    f = L.fq_pixel_shuffle_i8_nhwc
    x = torch.full((4096,), 0x33, dtype=torch.int8, device="cuda")
    y = torch.full((4096,), 0x55, dtype=torch.int8, device="cuda")
    p, p2 = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    good = (p, 16, p2, 16, 3, 2, 0, 1, 2, 2)
    rows = {
        "null x": ((None,) + good[1:], INVALID), "null y": (good[:2] + (None,) + good[3:], INVALID),
        "misaligned x": ((ctypes.c_void_p(p.value + 4),) + good[1:], INVALID),
        "misaligned y": (good[:2] + (ctypes.c_void_p(p2.value + 8),) + good[3:], INVALID),
        "N < 0": (good[:7] + (-1, 2, 2), INVALID), "H < 1": (good[:7] + (1, 0, 2), INVALID), "W < 1": (good[:7] + (1, 2, 0), INVALID),
        "C < 1": (good[:4] + (0,) + good[5:], INVALID), "inverse 2": (good[:6] + (2,) + good[7:], INVALID),
        "Cpad_in": ((p, 32) + good[2:], INVALID), "Cpad_out": (good[:3] + (32,) + good[4:], INVALID),
        "r = 1": (good[:5] + (1,) + good[6:], UNSUPPORTED), "r = 5": ((p, 80, p2, 16, 3, 5, 0, 1, 2, 2), UNSUPPORTED),
        "C r^2 > 65536": ((p, 65552, p2, 16400, 16385, 2, 0, 1, 1, 1), UNSUPPORTED),
        "an output of 2^31 bytes": (good[:7] + ((1 << 31) // 16 // 4, 1, 1), UNSUPPORTED),
        "a source of 2^31 bytes": ((p, 64, p2, 16, 16, 2, 0, (1 << 31) // 64, 1, 1), UNSUPPORTED),
        "N H W past 2^31": (good[:7] + (1, 1 << 20, 1 << 20), UNSUPPORTED),
        "a wrong scalar beats a null pointer": ((None, 16, None, 16, 3, 7, 0, 1, 2, 2), UNSUPPORTED),
    }
    for what, (a, code) in rows.items():
        assert f(*a, None) == code, what
    assert f(None, 16, None, 16, 3, 2, 0, 0, 2, 2, None) == 0                            # N == 0: FQ_OK without a launch
    torch.cuda.synchronize()
    assert bool((y == 0x55).all()) and bool((x == 0x33).all())
    t = torch.zeros(1, 2, 2, 64, dtype=torch.int8, device="cuda")
    for bad in ((t, 16, 5, 0), (t, 8, 2, 0), (t, 64, 3, 1), (t.cpu(), 16, 2, 0)):
        with pytest.raises((_native.FqError, AssertionError)):
            _native.pixel_shuffle_i8_nhwc(*bad)
    assert _native.pixel_shuffle_i8_nhwc(t[:0], 16, 2, 0).shape == (0, 4, 4, 16)
