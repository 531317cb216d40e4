"""Shared by tests/test_deconv_f32_cpu.py and tests/test_gpu_deconv_f32.py (test infrastructure, no product code): the shape list
of the transposed float convolution fq_deconv_f32, seeded operands, the float64 reference, and an emulator of the numerics
contract of include/fq.h -- per output ONE fmaf chain over the taps (r, s) of its phase, ascending, c innermost, from +0.0f, a
tap outside the image being the operand +0.0f, then acc + bias in fp32 -- evaluated with libm's fmaf through ctypes (about a
microsecond per call: shapes below 500 000 multiply-adds only)."""
import os
import re

import numpy as np
import torch

from grouped_f32_util import _fmaf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def max_blocks():
    """kDcMaxBlocks of csrc/fq_deconv_f32_geom.h: the largest grid the host launches."""
    geom = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_deconv_f32_geom.h")).read()
    return int(re.search(r"constexpr int kDcMaxBlocks = (\d+);", geom).group(1))


# N, Cin, Cout, H, W, R, S, stride, pad, outpad: a single source pixel; a kernel below the stride (three of four phases have no tap:
# bias only) with output padding; the paper's 2x2/2 on an odd plane, two images; the pix2pix geometry; the LinkNet geometry (phases
# with 4, 2, 2 and 1 taps); stride 1 (one phase); R != S at stride 3 with row phases without a tap and output padding 2; every
# limit at once; three K steps per tap and a partly filled row tile; one channel quad beyond a 128-row tile; an output row wider
# than any column tile
SHAPES = [(1, 16, 4, 1, 1, 2, 2, 2, 0, 0), (1, 16, 4, 1, 1, 1, 1, 2, 0, 1), (2, 16, 8, 3, 5, 2, 2, 2, 0, 0),
          (1, 16, 4, 5, 7, 4, 4, 2, 1, 0), (1, 16, 4, 5, 7, 3, 3, 2, 1, 1), (1, 16, 4, 4, 4, 3, 3, 1, 1, 0),
          (1, 32, 4, 3, 3, 2, 3, 3, 1, 2), (1, 16, 4, 2, 2, 8, 8, 4, 7, 3), (1, 48, 40, 4, 4, 2, 2, 2, 0, 0),
          (1, 16, 132, 3, 3, 2, 2, 2, 0, 0), (3, 16, 4, 2, 70, 2, 2, 2, 0, 0)]
CONTRACT_SHAPES = list(SHAPES)
# ... and, from the geometry header, more work items than the largest grid has workgroups: up to 32 output channels a work item is
# 128 columns of one row phase, and a 1x1 kernel at stride 4 has four row phases of N * H * W columns each
BIG = (4, 16, 4, 130, 130, 1, 1, 4, 0, 0)
SHAPES = SHAPES + [BIG]
IDS = ["x".join(map(str, s)) for s in SHAPES]
CONTRACT_IDS = ["x".join(map(str, s)) for s in CONTRACT_SHAPES]
CONTRACT_LIMIT = 500000


def work_items(shape):
    """Work items of a launch with at most 32 output channels (csrc/fq_deconv_f32_geom.h: dc_plan)."""
    N, _cin, cout, H, W, R, S, stride, pad, outpad = shape
    assert cout <= 32
    ho, wo = out_hw(shape)
    qmax = -(-wo // stride)
    return sum(-(-(N * -(-(ho - rp) // stride) * qmax) // 128) for rp in range(stride) if ho > rp)


def out_hw(shape):
    _N, _cin, _cout, H, W, R, S, stride, pad, outpad = shape
    return (H - 1) * stride - 2 * pad + R + outpad, (W - 1) * stride - 2 * pad + S + outpad


def macs(shape):
    """Multiply-adds the contract issues: every tap of every output's phase, the ones outside the image included."""
    N, cin, cout, _H, _W, R, S, stride, pad, _outpad = shape
    ho, wo = out_hw(shape)
    rows = sum(len(range((oh + pad) % stride, R, stride)) for oh in range(ho))
    cols = sum(len(range((ow + pad) % stride, S, stride)) for ow in range(wo))
    return N * cout * cin * rows * cols


def operands(shape, integer, seed=0):
    """(x, w, b) on the host, fp32; w in the module's layout [Cin][Cout][R][S].  integer: small integers, so that every partial
    sum is an integer (the caller asserts the bound below 2^24) and every fp32 sum is exact in any order; else Gaussian, the
    weights scaled to keep the outputs near 1."""
    N, cin, cout, H, W, R, S, stride, _pad, _outpad = shape
    g = torch.Generator().manual_seed(1000 * sum(shape) + 10 * seed + int(integer))
    if integer:
        x = torch.randint(-8, 9, (N, cin, H, W), generator=g).float()
        w = torch.randint(-4, 5, (cin, cout, R, S), generator=g).float()
        b = torch.randint(-100, 101, (cout,), generator=g).float()
    else:
        taps = max(1, -(-R // stride) * -(-S // stride))
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(cin, cout, R, S, generator=g) / (taps * cin) ** 0.5
        b = torch.randn(cout, generator=g)
    return x, w, b


def pack(w):
    """The module's weight [Cin][Cout][R][S] -> wt [(r*S + s)*Cin + c][Cout], as include/fq.h states it."""
    cin, cout, R, S = w.shape
    return w.permute(2, 3, 0, 1).reshape(R * S * cin, cout).contiguous()


def ref64(x, w, b, stride, pad, outpad):
    """float64 F.conv_transpose2d on the host (x, w, b: any device); returned on the host."""
    return torch.nn.functional.conv_transpose2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(),
                                                stride=stride, padding=pad, output_padding=outpad)


def emulate(x, w, b, stride, pad, outpad):
    """The numerics contract of fq_deconv_f32, literally.  x, w ([Cin][Cout][R][S]), b: host fp32 tensors (b may be None:
    acc + 0.0f)."""
    fmaf = _fmaf()
    N, cin, H, W = x.shape
    _cin, K, R, S = w.shape
    ho, wo = (H - 1) * stride - 2 * pad + R + outpad, (W - 1) * stride - 2 * pad + S + outpad
    xl, wl = x.tolist(), w.tolist()
    bias = np.zeros(K, np.float32) if b is None else b.numpy().astype(np.float32)
    y = np.empty((N, K, ho, wo), np.float32)
    for n in range(N):
        for k in range(K):
            for oh in range(ho):
                for ow in range(wo):
                    acc = 0.0
                    for r in range(R):
                        if (oh + pad - r) % stride:
                            continue
                        ih = (oh + pad - r) // stride
                        for s in range(S):
                            if (ow + pad - s) % stride:
                                continue
                            iw = (ow + pad - s) // stride
                            inside = 0 <= ih < H and 0 <= iw < W
                            for c in range(cin):
                                acc = fmaf(wl[c][k][r][s], xl[n][c][ih][iw] if inside else 0.0, acc)
                    y[n, k, oh, ow] = np.float32(acc) + bias[k]
    return torch.from_numpy(y)
