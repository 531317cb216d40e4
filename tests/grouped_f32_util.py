"""Shared by tests/test_grouped_f32_cpu.py and tests/test_gpu_grouped_f32.py (test infrastructure, no product code): the shape
list of the grouped float convolution fq_gconv_f32, seeded operands, the float64 reference, and an emulator of the numerics
contract of include/fq.h -- per output ONE fmaf chain over (r, s, c), c innermost, from +0.0f, a padded tap being the operand
+0.0f, then acc + bias in fp32 -- evaluated with libm's fmaf through ctypes (about a microsecond per call: shapes below
500 000 multiply-adds only)."""
import ctypes
import ctypes.util

import numpy as np
import torch

# N, groups, Cgi, Cgo, H, W, R, stride, pad: a single pixel (1x1 and 3x3), a 1x1 output, unequal channel counts, odd planes,
# pad = R - 1, many groups of 4, 32 and 64 per group (64 x 9 weights per channel: the output channels of a group go in chunks of
# 16), 1x1 kernels at both strides, a row wider and a plane taller than any tile; then, from csrc/fq_gconv_f32_geom.h: more tiles
# (33 x 64 units of one tile each) than the 2048 workgroups of the largest grid; a last channel chunk that is partly filled
# (40 = 16 + 16 + 8); two column blocks and two row bands at sizes the contract emulator can afford
SHAPES = [(1, 2, 4, 4, 1, 1, 1, 1, 0), (1, 2, 4, 4, 1, 1, 3, 1, 1), (2, 3, 4, 8, 3, 3, 3, 1, 0), (1, 2, 8, 4, 5, 7, 3, 2, 1),
          (3, 2, 12, 12, 7, 7, 3, 1, 1), (1, 2, 4, 4, 6, 6, 3, 1, 2), (2, 32, 4, 4, 14, 14, 3, 1, 1), (2, 2, 32, 32, 7, 7, 3, 1, 1),
          (1, 2, 64, 64, 6, 6, 3, 2, 1), (1, 4, 20, 36, 5, 5, 1, 2, 0), (2, 5, 4, 64, 4, 4, 1, 1, 0), (1, 2, 16, 16, 9, 300, 3, 1, 1),
          (1, 2, 16, 16, 300, 9, 3, 2, 1), (33, 64, 4, 4, 7, 7, 3, 1, 1), (1, 2, 64, 40, 3, 3, 3, 1, 1), (1, 2, 4, 4, 3, 70, 3, 1, 1),
          (1, 2, 64, 4, 24, 3, 3, 1, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
CONTRACT_LIMIT = 500000


def out_hw(shape):
    _N, _G, _cgi, _cgo, H, W, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def macs(shape):
    N, G, cgi, cgo, _H, _W, R, _stride, _pad = shape
    ho, wo = out_hw(shape)
    return N * G * cgo * ho * wo * cgi * R * R


CONTRACT_SHAPES = [s for s in SHAPES if macs(s) < CONTRACT_LIMIT]


def operands(shape, integer, seed=0):
    """(x, w, b) on the host, fp32.  integer: small integers, so that every partial sum is an integer (the caller asserts the
    bound below 2^24) and every fp32 sum is exact in any order; else Gaussian, the weights scaled to keep the outputs near 1."""
    N, G, cgi, cgo, H, W, R, _stride, _pad = shape
    g = torch.Generator().manual_seed(1000 * sum(shape) + 10 * seed + int(integer))
    if integer:
        x = torch.randint(-8, 9, (N, G * cgi, H, W), generator=g).float()
        w = torch.randint(-4, 5, (G * cgo, cgi, R, R), generator=g).float()
        b = torch.randint(-100, 101, (G * cgo,), generator=g).float()
    else:
        x = torch.randn(N, G * cgi, H, W, generator=g)
        w = torch.randn(G * cgo, cgi, R, R, generator=g) / (R * cgi ** 0.5)
        b = torch.randn(G * cgo, generator=g)
    return x, w, b


def ref64(x, w, b, groups, stride, pad):
    """float64 F.conv2d(groups=G) on the host (x, w, b: any device); returned on the host."""
    return torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), stride=stride,
                                      padding=pad, groups=groups)


_FMAF = None


def _fmaf():
    global _FMAF
    if _FMAF is None:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.fmaf.restype = ctypes.c_float
        libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
        assert libm.fmaf(3.0, 5.0, 1.0) == 16.0
        # one rounding, not two: (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24, which fp32 holds; the rounded product alone loses the 2^-24
        a = float(np.float32(1.0) + np.float32(2.0 ** -12))
        assert libm.fmaf(a, a, -1.0) == 2.0 ** -11 + 2.0 ** -24
        _FMAF = libm.fmaf
    return _FMAF


def emulate(x, w, b, groups, stride, pad):
    """The numerics contract of fq_gconv_f32, literally.  x, w, b: host fp32 tensors (b may be None: acc + 0.0f)."""
    fmaf = _fmaf()
    N, C, H, W = x.shape
    K, cgi, R, S = w.shape
    cgo = K // groups
    ho, wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad)                     # +0.0f where a tap leaves the image
    xp[:, :, pad:pad + H, pad:pad + W] = x
    xl, wl = xp.tolist(), w.tolist()
    bias = np.zeros(K, np.float32) if b is None else b.numpy().astype(np.float32)
    y = np.empty((N, K, ho, wo), np.float32)
    for n in range(N):
        for k in range(K):
            planes = xl[n][(k // cgo) * cgi:(k // cgo + 1) * cgi]
            wk = wl[k]
            for oh in range(ho):
                for ow in range(wo):
                    acc = 0.0
                    for r in range(R):
                        ih = oh * stride + r
                        for s in range(S):
                            iw = ow * stride + s
                            for c in range(cgi):
                                acc = fmaf(wk[c][r][s], planes[c][ih][iw], acc)
                    y[n, k, oh, ow] = np.float32(acc) + bias[k]
    return torch.from_numpy(y)
