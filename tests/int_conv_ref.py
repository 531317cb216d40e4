"""Exact integer expected values at sizes where the oracle's plain loops would take minutes (test infrastructure, no product code).

  conv2d_int_fast    the integer convolution of oracle.conv2d_int (groups == 1, zero padding) computed by torch's float64 CPU
                     convolution.  Operands are int8-valued, so every product is below 2^14 in magnitude and every partial sum,
                     in whatever order the library adds them, is an integer below R*S*C*2^14 < 2^53: float64 holds it exactly.
                     tests/test_int_conv_ref_cpu.py ties it to the oracle bit for bit on small shapes;
  add_resident_ref   fq_add_resident's expression (include/fq.h) in NumPy, for the fused residual add of the convolution kernels;
  first_difference   where two [N][K][P][Q] arrays differ first, as (n, k, p, q), the 128-pixel tile and the count.
"""
import numpy as np
import torch

THREADS = 16                         # a fixed pool: the host's core count says nothing about what this process may use


def conv2d_int_fast(x, w, stride=(1, 1), pad=(0, 0), dil=(1, 1)):
    """x [N][C][H][W], w [K][C][R][S]: integer arrays with int8-valued entries -> int64 [N][K][P][Q]."""
    x = np.asarray(x)
    w = np.asarray(w)
    assert x.ndim == 4 and w.ndim == 4 and x.shape[1] == w.shape[1], (x.shape, w.shape)
    assert np.issubdtype(x.dtype, np.integer) and np.issubdtype(w.dtype, np.integer)
    assert x.size == 0 or (-128 <= int(x.min()) and int(x.max()) <= 127), "activations are int8 valued"
    assert -128 <= int(w.min()) and int(w.max()) <= 127, "weights are int8 valued"
    K, C, R, S = w.shape
    assert R * S * C * 2 ** 14 < 2 ** 53, "the accumulator bound leaves float64's integers"
    assert x.size * 8 <= 2 ** 29, "the float64 copy of the input would pass 0.5 GB: use fewer images"
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, THREADS))
    try:
        with torch.no_grad():
            acc = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x)).double(),
                                             torch.from_numpy(np.ascontiguousarray(w)).double(), None,
                                             stride=tuple(stride), padding=tuple(pad), dilation=tuple(dil))
    finally:
        torch.set_num_threads(before)
    assert bool((acc == torch.round(acc)).all()) and float(acc.abs().max() if acc.numel() else 0.0) <= R * S * C * 2 ** 14
    return acc.to(torch.int64).numpy()


def add_resident_ref(x, gx, y, gy, g_wide, ib, relu):
    """include/fq.h, fq_add_resident: x, y integer arrays standing for x * 2^-gx and y * 2^-gy;
         s      = clamp(x * 2^-gx + y * 2^-gy, relu ? 0 : -128, 127)
         wide   = (int16) (s * 2^g_wide),  g_wide = max(0, gx, gy) <= 8
         narrow = (int8) clamp(rint(s * 2^ib), -128, 127)
    Returns (wide int16, narrow int8).  The reference evaluates s in fp32; the operands are multiples of 2^-g_wide below 2^16 in
    magnitude, so both terms, their sum and the two scalings are exact in fp32 and in the float64 used here alike."""
    assert g_wide == max(0, gx, gy) and g_wide <= 8
    s = np.asarray(x).astype(np.float64) * 2.0 ** -gx + np.asarray(y).astype(np.float64) * 2.0 ** -gy
    s = np.clip(s, 0.0 if relu else -128.0, 127.0)
    wide = s * 2.0 ** g_wide
    assert np.array_equal(wide, np.rint(wide)) and (np.abs(wide).max() if wide.size else 0) <= 32767
    narrow = np.clip(np.rint(s * 2.0 ** ib), -128.0, 127.0)         # (np.rint: halves to even, as rintf / torch.round)
    return wide.astype(np.int16), narrow.astype(np.int8)


def first_difference(got, ref, tile=128):
    """got, ref: [N][K][P][Q].  None when equal; else a sentence naming the first differing output in the kernels' pixel order
    (m = (n * P + p) * Q + q, then k), its tile m // tile, and how many outputs differ."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return "shape %s, expected %s" % (got.shape, ref.shape)
    bad = got != ref
    count = int(bad.sum())
    if not count:
        return None
    N, K, P, Q = ref.shape
    per_pixel = bad.transpose(0, 2, 3, 1).reshape(-1, K)             # [M][K]
    rows = per_pixel.any(axis=1)
    m = int(np.argmax(rows))
    k = int(np.argmax(per_pixel[m]))
    n, p, q = m // (P * Q), (m // Q) % P, m % Q
    tiles = np.unique(np.nonzero(rows)[0] // tile)
    ks = np.nonzero(per_pixel.any(axis=0))[0]
    return ("%d of %d outputs differ; first at (n, k, p, q) = (%d, %d, %d, %d), pixel tile m // %d = %d: got %s, expected %s; "
            "%d pixel tiles affected (first %d, last %d), channels %d..%d"
            % (count, bad.size, n, k, p, q, tile, m // tile, got[n, k, p, q], ref[n, k, p, q], tiles.size, tiles[0], tiles[-1],
               ks[0], ks[-1]))
