"""The closed form of the re-quantising concatenation (include/fq.h: fq_concat_rq_i8_nhwc) in NumPy -- test infrastructure, no
product code.  Written apart from the kernel's packed-int16 steps (csrc/fq_concat_i8_geom.h, crq_requant): the quotient, the
dropped bits compared with one half, the tie by the quotient's parity, in int64.

  requant(v, shift, relu)      integer array (any int8 / int16 value) -> int64 array in [-128, 127]
  concat_rq(srcs)              srcs = [(array [N, H / up, W / up, Cpad], C, up, relu, shift)] -> int8 [N, H, W, pad16(sum C)]
  ties(v, shift)               how many elements of v sit exactly between two integers after the shift
"""
import numpy as np


def pad16(c):
    return (int(c) + 15) // 16 * 16


def requant(v, shift, relu):
    v = np.asarray(v).astype(np.int64)
    shift = int(shift)
    if shift >= 0:
        r = v * (1 << shift)
    else:
        k = -shift
        q, rem, half = v >> k, v & ((1 << k) - 1), 1 << (k - 1)
        r = q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(np.int64)
    if relu:
        r = np.maximum(r, 0)
    return np.clip(r, -128, 127)


def ties(v, shift):
    if shift >= 0:
        return 0
    k = -int(shift)
    return int(((np.asarray(v).astype(np.int64) & ((1 << k) - 1)) == (1 << (k - 1))).sum())


def concat_rq(srcs):
    total = sum(int(C) for _a, C, _up, _relu, _shift in srcs)
    a0, _C, up0 = srcs[0][0], srcs[0][1], int(srcs[0][2])
    N, H, W = a0.shape[0], a0.shape[1] * up0, a0.shape[2] * up0
    out = np.zeros((N, H, W, pad16(total)), dtype=np.int8)
    base = 0
    for a, C, up, relu, shift in srcs:
        C, up = int(C), int(up)
        assert a.dtype in (np.int8, np.int16) and a.shape[0] == N and a.shape[1] * up == H and a.shape[2] * up == W and a.shape[3] % 16 == 0
        big = np.repeat(np.repeat(a[..., :C], up, axis=1), up, axis=2)
        out[..., base:base + C] = requant(big, shift, relu).astype(np.int8)
        base += C
    return out
