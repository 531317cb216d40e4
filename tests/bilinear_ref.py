"""The closed form of the resident int8 bilinear upsampling (include/fq.h: fq_upsample_bilinear_i8_nhwc) in NumPy -- test
infrastructure, no product code.  Plain integers throughout: int64 sums, one rounding half to even done with integer arithmetic.

  taps(size, up)               (i0, i1, l0, l1) per output index along one axis of `size` source elements
  sums(x, up)                  S = sum over the 2 x 2 taps of ly lx q, int64 [N, up H, up W, C], from x int8 [N, H, W, C]
  requant(S, up, shift, relu)  clamp(relu ? max(r, 0) : r, -128, 127), r = S 2^(shift - 2 log2(2 up)) rounded half to even
  upsample(x, c, up, shift, relu)   the entry point's result on x int8 [N, H, W, Cpad] with c real channels: padding channels zero
"""
import numpy as np


def pad16(c):
    return (int(c) + 15) // 16 * 16


def taps(size, up):
    o = np.arange(up * size, dtype=np.int64)
    D = 2 * up
    t = np.maximum(2 * o + 1 - up, 0)
    i0 = t // D
    l1 = t % D
    return i0, np.minimum(i0 + 1, size - 1), D - l1, l1


def sums(x, up):
    q = x.astype(np.int64)
    r0, r1, a0, a1 = taps(q.shape[1], up)
    c0, c1, b0, b1 = taps(q.shape[2], up)
    rows = q[:, r0] * a0[None, :, None, None] + q[:, r1] * a1[None, :, None, None]
    return rows[:, :, c0] * b0[None, None, :, None] + rows[:, :, c1] * b1[None, None, :, None]


def requant(S, up, shift, relu):
    e = int(shift) - 2 * int(np.log2(2 * up))
    S = S.astype(np.int64)
    if e >= 0:
        r = S * (1 << e)
    else:
        k = -e
        floor = S >> k                                      # (arithmetic: floor for negative sums too)
        rem = S - (floor << k)
        half = 1 << (k - 1)
        r = floor + ((rem > half) | ((rem == half) & ((floor & 1) == 1)))
    if relu:
        r = np.maximum(r, 0)
    return np.clip(r, -128, 127).astype(np.int8)


def upsample(x, c, up, shift, relu):
    y = np.zeros((x.shape[0], up * x.shape[1], up * x.shape[2], x.shape[3]), dtype=np.int8)
    y[..., :c] = requant(sums(x[..., :c], up), up, shift, relu)
    return y
