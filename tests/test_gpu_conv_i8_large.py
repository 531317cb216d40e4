"""The int8 convolution kernels on the launches that fill the chip, against an exact reference.

conv2d_i8_dispatch (csrc/fq_conv_i8.hip) picks 128-row output tiles, the ring of two, the eight-wave halo kernel and more tiles
than the persistent 64-channel kernel has workgroups only when the launch covers the 256 CUs -- M * K of a few million.  The
oracle's plain loops take minutes there, so these rows take their expected accumulator from tests/int_conv_ref.py (a float64
convolution, exact for int8 operands and tied to the oracle by tests/test_int_conv_ref_cpu.py) and then the oracle's own tail.
Every row states the kernel it must reach NATURALLY -- no FQ_* switch -- and the variant log decides whether it did; every
comparison is exact equality and a mismatch names the first differing (n, k, p, q) and its 128-pixel tile.
The partial-tile masks of the 128-row forms at small K: tests/test_gpu_fuzz.py with FQ_CONV_TK=128.   pytest -m gpu"""
import collections
import zlib

import numpy as np
import pytest
import torch

from int_conv_ref import add_resident_ref, conv2d_int_fast, first_difference
from per_channel_chain import pc_epilogue

OB = 3

# name; variant: the kernel of the plain call; add_variant: the kernel of the call with a fused residual add (the halo and c64
# kernels decline a residual: the layer then runs on the LDS-DMA or the 64-channel tile kernel); rs: the integer-tail shift
Case = collections.namedtuple("Case", "name variant add_variant N C H W K R S stride pad rs")
CASES = [Case(*c) for c in (
    ("tile_c128_128", "tile_c128/128", "tile_c128/128", 32, 128, 32, 32, 256, 1, 1, 1, 0, 11),
    ("tile_c128_128_ragged", "tile_c128/128", "tile_c128/128", 33, 128, 31, 33, 256, 1, 1, 1, 0, 11),   # 263.7 pixel tiles
    ("tile_c64_128_ragged", "tile_c64/128", "tile_c64/128", 23, 64, 56, 56, 256, 1, 1, 1, 0, 10),       # 563.5 pixel tiles
    ("tile_c64_128_k200", "tile_c64/128", "tile_c64/128", 12, 64, 56, 56, 200, 1, 1, 1, 0, 10),         # partial second k tile
    ("tile_c64_128_3x3_s2", "tile_c64/128", "tile_c64/128", 36, 64, 56, 56, 256, 3, 3, 2, 1, 12),       # nine taps, two per K-step
    ("tile_general_128_k160", "tile_general/128", "tile_general/128", 8, 48, 64, 64, 160, 1, 1, 1, 0, 10),
    ("tile_general_128_3x3_k200", "tile_general/128", "tile_general/128", 9, 48, 61, 61, 200, 3, 3, 1, 1, 11),
    ("dma2_64", "dma2/64", "dma2/64", 40, 128, 64, 64, 64, 3, 3, 2, 1, 12),
    ("dma2_64_ragged", "dma2/64", "dma2/64", 41, 128, 62, 66, 64, 3, 3, 2, 1, 12),                      # 31 x 33 outputs, 327.7 tiles
    ("dma2_128", "dma2/128", "dma2/128", 9, 1024, 56, 56, 256, 1, 1, 1, 0, 12),                         # 220.5 pixel tiles
    ("dma2_128_3x3_s2", "dma2/128", "dma2/128", 40, 128, 64, 64, 256, 3, 3, 2, 1, 12),
    ("dma3_128", "dma3/128", "dma3/128", 16, 128, 64, 64, 256, 3, 3, 2, 1, 12),                         # exactly 256 workgroups
    ("dma3_128_ragged", "dma3/128", "dma3/128", 16, 128, 60, 68, 256, 3, 3, 2, 1, 12),                  # 30 x 34 outputs, 127.5 tiles
    ("halo_128", "halo/128", "dma2/128", 12, 128, 56, 56, 128, 3, 3, 1, 1, 12),
    ("halo_128_ragged", "halo/128", "dma2/128", 13, 128, 55, 53, 128, 3, 3, 1, 1, 12),
    ("halo8_64", "halo8/64", "dma2/64", 64, 128, 32, 32, 64, 3, 3, 1, 1, 12),
    ("halo8_64_ragged", "halo8/64", "dma2/64", 64, 128, 31, 33, 64, 3, 3, 1, 1, 12),                    # tiles span images
    ("halo8_128", "halo8/128", "dma2/128", 43, 128, 28, 28, 256, 3, 3, 1, 1, 12),
    ("c64_halo", "c64_halo/64", "tile_c64/64", 23, 64, 56, 56, 64, 3, 3, 1, 1, 12),                     # 564 tiles, 512 workgroups
    ("c64_halo_k48", "c64_halo/64", "tile_c64/64", 23, 64, 56, 56, 48, 3, 3, 1, 1, 12),
)]
IDS = [c.name for c in CASES]

WANTED = {"tile_c128/128", "tile_c64/128", "tile_general/128", "dma2/64", "dma2/128", "dma3/128", "halo/128", "halo8/64",
          "halo8/128", "c64_halo/64"}


def _geom(c):
    """(output pixels M, output pixels of one image)"""
    P, Q = (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1
    return c.N * P * Q, P * Q


def _shape(c):
    return (c.N, c.C, c.H, c.W, c.K, c.R, c.S, c.stride, c.pad)


def test_the_case_list_covers_what_it_claims():
    import test_gpu_per_channel_weights as pcw
    assert len(set(IDS)) == len(CASES) and len({_shape(c) for c in CASES}) == len(CASES)
    assert {c.variant for c in CASES} >= WANTED
    general = [c for c in CASES if c.variant == "tile_general/128"]
    assert all(c.K % 128 for c in general) and {(c.R, c.S) for c in general} >= {(1, 1), (3, 3)}     # a partial second 128-tile
    assert any(c.variant == "tile_c64/128" and c.K % 128 for c in CASES)
    for variant in sorted(WANTED):                                                                   # kernel by kernel
        rows = [c for c in CASES if c.variant == variant]
        assert any(_geom(c)[0] % 128 for c in rows), variant                                         # a partial last pixel tile
        assert any(_geom(c)[1] % 128 and 128 % _geom(c)[1] for c in rows), variant                   # tiles straddle images
    assert any(c.variant == "halo8/64" and _geom(c)[0] % 256 and (c.H, c.W) == (31, 33) for c in CASES)
    c64 = [c for c in CASES if c.variant == "c64_halo/64"]
    assert all((_geom(c)[0] + 127) // 128 > 512 for c in c64) and {c.K for c in c64} >= {64, 48}     # workgroups loop over tiles
    dma3 = [c for c in CASES if c.variant == "dma3/128"]
    assert dma3 and all((_geom(c)[0] + 127) // 128 * (c.K // 128) == 256 for c in dma3)
    # the fused residual add runs on the tile and LDS-DMA kernels, 128-row forms included
    assert {c.add_variant for c in CASES} >= {"tile_c128/128", "tile_c64/128", "tile_general/128", "dma2/64", "dma2/128", "dma3/128"}
    # what test_gpu_per_channel_weights.py can only compare with the per-tensor kernel is compared with the oracle here
    mine = {_shape(c) for c in CASES}
    large = [s for s in pcw.SHAPES if not s[11]]
    assert len(large) >= 4
    for _name, N, H, W, C, K, R, S, st, pd, _variant, _small in large:
        assert (N, C, H, W, K, R, S, st, pd) in mine, _name
    assert all(c.N * c.C * c.H * c.W * 8 < 2 ** 29 for c in CASES)                                   # the float64 copy of the input
    assert all(1 <= c.rs <= 16 for c in CASES)


class _Row(object):
    pass


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def row(request, oracle):
    """One row's operands, exact accumulator and device tensors, built once for the tests of that row."""
    from common.quantity import _native as nat
    nat.lib()
    r = _Row()
    r.nat, r.oracle = nat, oracle
    c = request.param
    r.name, r.variant, r.add_variant, r.rs = c.name, c.variant, c.add_variant, c.rs
    N, C, H, W, K, R, S, st, pd = _shape(c)
    r.K, r.kpad = K, (K + 15) // 16 * 16
    rng = _rng(r.name, "operands")
    x = rng.integers(-128, 128, size=(N, C, H, W)).astype(np.int8)
    w = rng.integers(-128, 128, size=(K, C, R, S)).astype(np.int8)
    x.reshape(-1)[::11] = -128
    w.reshape(-1)[::7] = -128                                          # (-128) * (-128) products in every sum
    assert len({img.tobytes() for img in x}) == N                      # no two images equal
    qb = rng.integers(-128, 128, size=K).astype(np.float32)
    qb[::7] = [(-1) ** i * v for i, v in enumerate(np.resize([300.0, 1e5, 3e9, 40000.0, 255.0, 256.0], len(qb[::7])))]
    acc = conv2d_int_fast(x, w, (st, st), (pd, pd), (1, 1))
    assert np.abs(acc).max() < 2 ** 24                                 # (so the fp32 copy below is the accumulator itself)
    r.acc = acc.astype(np.float32)
    r.qb = qb
    r.geom = ((st, st), (pd, pd), (1, 1))
    r.x = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
    r.w = nat.pack_weight_krsc(torch.from_numpy(w.astype(np.float32)).cuda())
    assert tuple(r.w.shape) == (K, R, S, C)
    r.b = torch.from_numpy(qb).cuda()
    return r


def _rng(row_name, use):
    """One generator per row and use, so a test draws the same data whichever tests ran before it."""
    return np.random.default_rng(zlib.crc32(("%s/%s" % (row_name, use)).encode()))


def _logged(r, variant, fn, *args):
    r.nat.conv_variant_log = log = {}
    try:
        out = fn(*args)
    finally:
        r.nat.conv_variant_log = None
    assert log == {variant: 1}, "%s ran %s, the table says %s" % (r.name, log, variant)
    return out


def _same(got, ref, what):
    msg = first_difference(got, ref)
    assert msg is None, "%s: %s" % (what, msg)


def _nchw(q, K):
    """int NHWC [N][P][Q][Kpad] device tensor -> (real channels as NCHW ndarray, padding channels)."""
    a = q.cpu().numpy()
    return a[..., :K].transpose(0, 3, 1, 2), a[..., K:]


@pytest.mark.gpu
def test_fp32_output_equals_the_exact_reference(row):
    r = row
    for rs in (r.rs, 17):                                              # the integer tail; the reference's fp32 chain (rs > 16)
        got = _logged(r, r.variant, r.nat.conv2d_i8, r.x, r.w, r.b, *r.geom, rs, OB).cpu().numpy()
        _same(got, r.oracle.recon_epilogue(r.acc, r.qb, rs, OB), "%s fp32 NCHW rs=%d" % (r.name, rs))


@pytest.mark.gpu
def test_resident_outputs_equal_the_exact_reference(row):
    r = row
    for rs, relu, want_f32 in ((r.rs, False, False), (r.rs, True, False), (r.rs, False, True), (r.rs, True, True), (17, True, False)):
        what = "%s resident rs=%d relu=%d fp32=%d" % (r.name, rs, relu, want_f32)
        y, q = _logged(r, r.variant, r.nat.conv2d_i8_resident, r.x, r.w, r.b, *r.geom, rs, OB, want_f32, True, relu)
        ref = r.oracle.recon_epilogue(r.acc, r.qb, rs, OB)
        if relu:
            ref = np.maximum(ref, np.float32(0))
        assert (y is not None) == want_f32
        if want_f32:
            _same(y.cpu().numpy(), ref, what + ", fp32 NCHW")
        assert tuple(q.shape) == (ref.shape[0], ref.shape[2], ref.shape[3], r.kpad)
        real, padding = _nchw(q, r.K)
        _same(real, r.oracle.quantity(ref, OB).astype(np.int8), what + ", int8 NHWC")
        assert not padding.any(), what + ": channels [K, Kpad) must be zero"


@pytest.mark.gpu
def test_fused_residual_add_equals_the_exact_reference(row):
    """fq_conv2d_i8_add_resident on the kernel that takes the row's layer when it ends a block: the convolution's int8 result
    (the tail at ob = 0 gives the integers) and the residual through fq_add_resident's expression."""
    r = row
    conv_q = r.oracle.recon_epilogue(r.acc, r.qb, r.rs, 0).astype(np.int32)          # [N][K][P][Q], value conv_q * 2^-OB
    N, K, P, Q = conv_q.shape
    ib = 4
    rng = _rng(r.name, "residuals")
    for res_dtype, g_res, relu, want_wide in ((np.int8, 5, True, True), (np.int16, 6, False, True), (np.int8, 2, True, False)):
        what = "%s fused add, %s residual g_res=%d relu=%d" % (r.name, res_dtype.__name__, g_res, relu)
        lim = 128 * 2 ** g_res if res_dtype == np.int16 else 128
        res = np.zeros((N, P, Q, r.kpad), dtype=res_dtype)
        res[..., :K] = rng.integers(-lim, lim, size=(N, P, Q, K))
        g = max(0, OB, g_res)
        wide_ref, narrow_ref = add_resident_ref(conv_q, OB, res[..., :K].transpose(0, 3, 1, 2), g_res, g, ib, relu)
        wide, narrow = _logged(r, r.add_variant, r.nat.conv2d_i8_add_resident, r.x, r.w, r.b, *r.geom, r.rs, OB,
                               torch.from_numpy(res).cuda(), g_res, want_wide, g, True, ib, relu)
        assert (wide is not None) == want_wide
        if want_wide:
            real, padding = _nchw(wide, K)
            _same(real, wide_ref, what + ", wide")
            assert not padding.any(), what + ": wide channels [K, Kpad) must be zero"
        real, padding = _nchw(narrow, K)
        _same(real, narrow_ref, what + ", narrow")
        assert not padding.any(), what + ": narrow channels [K, Kpad) must be zero"


@pytest.mark.gpu
def test_per_channel_shifts_equal_the_exact_reference(row):
    """The _pcs entry points with a spread shift vector against the per-channel tail on the same exact accumulator: every shift in
    the integer tail's range (fp32 output), and a spread that leaves it (int8 output with the ReLU)."""
    r = row
    nat = r.nat
    rng = _rng(r.name, "shift spreads")

    def spread(lo, hi):
        rs = rng.integers(lo, hi + 1, r.K).tolist()
        rs[0], rs[-1] = lo, hi
        return rs, nat.ShiftVec(torch.tensor(rs, dtype=torch.int32, device="cuda"), lo, hi)

    rs, vec = spread(max(1, r.rs - 4), min(16, r.rs + 4))
    got = _logged(r, r.variant, nat.conv2d_i8, r.x, r.w, r.b, *r.geom, vec, OB).cpu().numpy()
    _same(got, pc_epilogue(r.acc, r.qb, rs, OB), "%s per-channel shifts %d..%d, fp32 NCHW" % (r.name, min(rs), max(rs)))
    rs, vec = spread(r.rs - 3, 18)
    _y, q = _logged(r, r.variant, nat.conv2d_i8_resident, r.x, r.w, r.b, *r.geom, vec, OB, False, True, True)
    ref = np.maximum(pc_epilogue(r.acc, r.qb, rs, OB), np.float32(0))
    real, padding = _nchw(q, r.K)
    _same(real, r.oracle.quantity(ref, OB).astype(np.int8), "%s per-channel shifts %d..%d, int8 NHWC" % (r.name, min(rs), max(rs)))
    assert not padding.any()
