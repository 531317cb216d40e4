"""fq_upsample_bilinear_i8_nhwc on the GPU against its closed form in NumPy (tests/bilinear_ref.py), which
tests/test_bilinear_plan_cpu.py holds against the reference's chain DeQuantity -> F.interpolate -> ReLU -> Quantity (DESIGN section
30).  Exact.    pytest -m gpu"""
import numpy as np
import pytest
import torch

import bilinear_nets as bn
import bilinear_ref as br

pytestmark = pytest.mark.gpu

PLANES = bn.KERNEL_PLANES + (bn.BIG_PLANE,)


def _source(rng, n, h, w, c):
    """int8 [n, h, w, pad16(c)], garbage in the padding channels too."""
    return rng.integers(-128, 128, (n, h, w, br.pad16(c))).astype(np.int8)


def _run(nat, x, c, up, shift, relu):
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((x.shape[0], up * x.shape[1], up * x.shape[2], x.shape[3]), 0x55, dtype=torch.int8, device="cuda")
    assert nat.upsample_bilinear_i8_nhwc(xd, c, up, shift, relu, out=yd) is yd
    return yd.cpu().numpy()


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("up", (2, 4))
def test_the_kernel_is_the_closed_form(up, plane):
    """N in {1, 3}, C in {1, 16, 19, 33, 80}, shift in {-8, -3, -1, 0, 2, 5, 8}, ReLU on and off; the 33 x 47 plane takes more than
    one workgroup at every channel count."""
    from common.quantity import _native as nat
    rng = np.random.default_rng(1000 * up + 10 * plane[0] + plane[1])
    for n in (1, 3):
        for c in bn.KERNEL_CHANNELS:
            x = _source(rng, n, plane[0], plane[1], c)
            S = br.sums(x[..., :c], up)
            if plane == bn.BIG_PLANE:
                assert n * plane[0] * plane[1] * (br.pad16(c) // 16) > 256
            for shift in bn.KERNEL_SHIFTS:
                for relu in (False, True):
                    got = _run(nat, x, c, up, shift, relu)
                    want = br.requant(S, up, shift, relu)
                    np.testing.assert_array_equal(got[..., :c], want, err_msg=str((n, plane, c, up, shift, relu)))
                    assert not got[..., c:].any(), (n, plane, c, up, shift, relu)


@pytest.mark.parametrize("up", (2, 4))
def test_ties_saturation_and_the_checkerboard(up):
    from common.quantity import _native as nat
    c, cpad = 19, 32
    # constant planes of odd values at shift -1: S = D^2 q, r = q / 2 -- every output is a tie, and the floors have both parities
    odd = np.arange(-127, 128, 2).astype(np.int8)
    x = np.empty((len(odd), 3, 2, cpad), np.int8)
    x[...] = odd[:, None, None, None]
    got = _run(nat, x, c, up, -1, False)
    want = br.upsample(x, c, up, -1, False)
    np.testing.assert_array_equal(got, want)
    floors = np.floor(odd.astype(np.float64) / 2).astype(np.int64)
    assert set(floors % 2) == {0, 1}
    even = 2 * np.round(odd.astype(np.float64) / 4)          # half to even of q / 2 for odd q
    assert (got[:, 0, 0, 0] == even).all() and (got[..., :c] == even[:, None, None, None]).all() and not got[..., c:].any()
    # +-extreme planes with a positive shift: saturation both ways (and zero under the ReLU for the negative plane)
    for value in (-128, 127, -100, 100):
        x = np.full((1, 7, 9, cpad), value, np.int8)
        for shift in (2, 5, 8):
            for relu in (False, True):
                got = _run(nat, x, c, up, shift, relu)
                np.testing.assert_array_equal(got, br.upsample(x, c, up, shift, relu))
                assert (got[..., :c] == (127 if value > 0 else (0 if relu else -128))).all()
    # the checkerboard of -128 / 127, every shift
    board = np.where((np.add.outer(np.arange(7), np.arange(9)) % 2) == 0, -128, 127).astype(np.int8)
    x = np.broadcast_to(board[None, :, :, None], (2, 7, 9, cpad)).copy()
    x[..., c:] = 85                                          # (garbage in the padding channels)
    for shift in bn.KERNEL_SHIFTS:
        for relu in (False, True):
            np.testing.assert_array_equal(_run(nat, x, c, up, shift, relu), br.upsample(x, c, up, shift, relu), err_msg=str((shift, relu)))


def test_the_binding_allocates_the_output_and_refuses_what_the_entry_point_refuses():
    from common.quantity import _native as nat
    rng = np.random.default_rng(5)
    x = _source(rng, 2, 5, 6, 20)
    y = nat.upsample_bilinear_i8_nhwc(torch.from_numpy(x).cuda(), 20, 2, 0, False)
    assert tuple(y.shape) == (2, 10, 12, 32) and y.dtype == torch.int8
    np.testing.assert_array_equal(y.cpu().numpy(), br.upsample(x, 20, 2, 0, False))
    with pytest.raises(nat.FqError):
        nat.upsample_bilinear_i8_nhwc(torch.from_numpy(x), 20, 2, 0, False)              # a host tensor
    for up, shift in ((3, 0), (2, 9), (4, -9), (8, 0)):
        assert not nat.upsample_bilinear_supported(up, shift)
        with pytest.raises(nat.FqError):
            nat.upsample_bilinear_i8_nhwc(torch.from_numpy(x).cuda(), 20, up, shift, False)
    xd = torch.from_numpy(x).cuda()
    fn = nat.lib().fq_upsample_bilinear_i8_nhwc
    assert fn(xd.data_ptr(), xd.data_ptr(), 1, 2, 3, 20, 32, 2, 0, 0, nat._stream(xd)) == -1      # y overlaps x: invalid argument
    assert fn(None, None, 0, 5, 6, 20, 32, 2, 0, 0, nat._stream(xd)) == 0                         # N == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xd.cpu().numpy(), x)


def _torch_closed_form(x, c, up, shift, relu):
    """The closed form with torch integer ops on the device (int32): for the case whose NumPy reference would take minutes."""
    q = x[..., :c].to(torch.int32)
    dev = x.device

    def taps(size):
        i0, i1, l0, l1 = br.taps(size, up)
        return [torch.from_numpy(a).to(dev) for a in (i0, i1)] + [torch.from_numpy(a.astype(np.int32)).to(dev) for a in (l0, l1)]

    r0, r1, a0, a1 = taps(q.shape[1])
    c0, c1, b0, b1 = taps(q.shape[2])
    rows = q[:, r0] * a0[None, :, None, None] + q[:, r1] * a1[None, :, None, None]
    S = rows[:, :, c0] * b0[None, None, :, None] + rows[:, :, c1] * b1[None, None, :, None]
    e = shift - 2 * int(np.log2(2 * up))
    if e >= 0:
        r = S << e
    else:
        k = -e
        floor = S >> k
        rem = S - (floor << k)
        half = 1 << (k - 1)
        r = floor + ((rem > half) | ((rem == half) & ((floor & 1) == 1))).to(torch.int32)
    if relu:
        r = r.clamp_min(0)
    y = torch.zeros(x.shape[0], up * x.shape[1], up * x.shape[2], x.shape[3], dtype=torch.int8, device=dev)
    y[..., :c] = r.clamp(-128, 127).to(torch.int8)
    return y


def test_the_device_closed_form_is_the_numpy_one():
    rng = np.random.default_rng(9)
    x = _source(rng, 2, 7, 9, 19)
    for up in (2, 4):
        for shift in bn.KERNEL_SHIFTS:
            for relu in (False, True):
                got = _torch_closed_form(torch.from_numpy(x).cuda(), 19, up, shift, relu).cpu().numpy()
                np.testing.assert_array_equal(got, br.upsample(x, 19, up, shift, relu))


def test_an_output_just_below_2_31_bytes_and_one_just_above():
    """up 2 on a 4096 x 8191 plane of 16 bytes: the output is 2 147 221 504 bytes, 262 142 bytes under the limit of 2^31 - 2 (one more
    column is over it and is refused).  Checked band by band against the closed form in torch integer ops on the device."""
    from common.quantity import _native as nat
    h, w, c, cpad, up = 4096, 8191, 11, 16, 2
    out_bytes = up * up * h * w * cpad
    assert out_bytes <= (1 << 31) - 2 < up * up * h * (w + 1) * cpad
    need = out_bytes + h * w * cpad + (3 << 30)              # output, source, the reference's temporaries of one band
    free, _total = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the case needs %.1f GiB (+ 1 GiB for the allocator); %.1f GiB are free on this device" % (need / 2.0 ** 30, free / 2.0 ** 30))
    gen = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randint(-128, 128, (1, h, w, cpad), dtype=torch.int8, device="cuda", generator=gen)
    y = torch.full((1, up * h, up * w, cpad), 0x55, dtype=torch.int8, device="cuda")
    over = torch.empty(0, dtype=torch.int8, device="cuda")
    rc = nat.lib().fq_upsample_bilinear_i8_nhwc(x.data_ptr(), y.data_ptr(), 1, h, w + 1, c, cpad, up, -1, 0, nat._stream(x))
    assert rc == -4 and over.numel() == 0 and bool((y[0, 0, 0] == 0x55).all())          # refused on the host: nothing written
    nat.upsample_bilinear_i8_nhwc(x, c, up, -1, True, out=y)
    band = 128
    for a in range(0, h, band):
        b = min(a + band, h)
        lo, hi = max(a - 1, 0), min(b + 1, h)
        want = _torch_closed_form(x[:, lo:hi], c, up, -1, True)[:, up * (a - lo):up * (a - lo) + up * (b - a)]
        assert torch.equal(y[:, up * a:up * b], want), "source rows %d .. %d" % (a, b)
    assert bool((y[0, -1, -1, c:] == 0).all())
