"""Oracle-backed doubles for the grouped entry points of common.quantity._native (gconv2d_i8_resident, pack_weight_grouped), on
top of tests/depthwise_doubles.py -- so that the CPU suite can run a ResNeXt-style network with and without the grouped plan --
and the shape list that the GPU kernel test and the geometry walker (scripts/gconv_geom_check.cpp) share.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The grouped double follows the reference's chain
literally: grouped integer convolution (oracle.conv2d_int(groups=G)) -> RightShift -> BiasAdd -> Sp -> DeQuantity -> nn.ReLU ->
the next layer's Quantity(ob); a per-channel shift goes through per_channel_chain.pc_epilogue.
"""
import contextlib

import numpy as np
import torch

import depthwise_doubles
import native_doubles
from oracle import fq_oracle as orc

_np = native_doubles._np

# (groups, input channels per group, output channels per group)
GROUP_WIDTHS = [(2, 4, 4), (8, 4, 4), (3, 8, 4), (2, 16, 8), (2, 32, 32), (2, 64, 64), (5, 4, 12), (32, 4, 4)]
PLANES = [(1, 1), (2, 2), (5, 7), (9, 11), (33, 17)]
BATCHES = (1, 3)
# one launch with more strip blocks than the 2048 workgroups can take in one step
MANY_TILES = (32, 4, 4, 3, 1, 1, 8, 112, 112)


def kernel_shapes():
    """(G, Cgi, Cgo, R, stride, pad, N, H, W): the widths x {1x1, 3x3} x stride {1, 2} x every padding below R x the planes x
    N in {1, 3}, then MANY_TILES.  A plane smaller than the kernel without enough padding stays in the list: the entry point
    answers FQ_ERR_INVALID_ARG there."""
    out = []
    for (G, cgi, cgo) in GROUP_WIDTHS:
        for R in (1, 3):
            for stride in (1, 2):
                for pad in range(R):
                    for (H, W) in PLANES:
                        for N in BATCHES:
                            out.append((G, cgi, cgo, R, stride, pad, N, H, W))
    out.append(MANY_TILES)
    return out


def pack_weight_grouped(w, groups, kpad=None):
    """include/fq.h, written out byte by byte: unit ((kq * R*S + t) * (Cgi / 4) + j4), byte 4 * i + c = w[4 kq + i][4 j4 + c][t]."""
    a = _np(w)
    K, cgi, R, S = a.shape
    kpad = native_doubles.pad16(K) if kpad is None else int(kpad)
    out = np.zeros((kpad // 4, R * S, cgi // 4, 4, 4), dtype=np.int8)
    for k in range(K):
        for j in range(cgi):
            out[k // 4, :, j // 4, k % 4, j % 4] = a[k, j].reshape(-1).astype(np.int8)
    return torch.from_numpy(out)


def unpack_weight_grouped(wq, K):
    """int8 [Kpad / 4, R*S, Cgi / 4, 4, 4] -> int32 [K, Cgi, R, R]"""
    a = _np(wq).astype(np.int32)
    kq, taps, ch = a.shape[:3]
    R = int(round(taps ** 0.5))
    w = np.transpose(a, (0, 3, 2, 4, 1)).reshape(kq * 4, ch * 4, R, R)
    return np.ascontiguousarray(w[:K])


def gconv2d_i8_resident(xq, wq, qbias, K, groups, stride, padding, rs, ob, relu):
    w = unpack_weight_grouped(wq, K)
    C = groups * w.shape[1]
    x = np.ascontiguousarray(np.moveaxis(_np(xq).astype(np.int32), -1, 1)[:, :C])                  # NCHW, real channels
    acc = orc.conv2d_int(x, w, tuple(stride), tuple(padding), (1, 1), groups=groups)
    y = depthwise_doubles._tail(acc, qbias, depthwise_doubles._shifts(rs, K), ob)
    if relu:
        y = np.maximum(y, np.float32(0))
    return native_doubles._to_i8_nhwc(y, ob, native_doubles.pad16(K))


_DOUBLES = dict(pack_weight_grouped=pack_weight_grouped, gconv2d_i8_resident=gconv2d_i8_resident)


@contextlib.contextmanager
def installed():
    """depthwise_doubles.installed() plus the doubles above.  _native.gconv_supported stays the library's own: it is host
    arithmetic (fq_gconv2d_i8_supported) and needs no GPU."""
    with depthwise_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
