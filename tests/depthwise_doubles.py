"""Oracle-backed doubles for the depthwise entry points of common.quantity._native (dwconv2d_i8_resident, pack_weight_dw), on top
of tests/native_doubles.py, plus the two fp32 element-wise entry points the reference-shaped form of a grouped convolution needs
(recon_epilogue) -- so that the CPU suite can run a separable network with and without the depthwise plan.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The depthwise double follows the reference's chain
literally: grouped integer convolution (oracle.conv2d_int(groups=C)) -> RightShift -> BiasAdd -> Sp -> DeQuantity -> nn.ReLU ->
the next layer's Quantity(ob); a per-channel shift goes through per_channel_chain.pc_epilogue.
"""
import contextlib

import numpy as np
import torch

import native_doubles
import per_channel_chain as pcc
from oracle import fq_oracle as orc

_np = native_doubles._np


def _shifts(rs, C):
    """An int, or the C shifts of a ShiftVec-like object (attribute t)."""
    t = getattr(rs, "t", None)
    return int(rs) if t is None else [int(v) for v in _np(t)[:C]]


def _tail(acc, qbias, rs, ob):
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    qb = _np(qbias).astype(np.float32)
    if isinstance(rs, list):
        return pcc.pc_epilogue(acc, qb, rs, ob)
    return orc.recon_epilogue(acc, qb, rs, ob)


def pack_weight_dw(w, cpad=None):
    C, one, R, S = w.shape
    assert one == 1
    cpad = native_doubles.pad16(C) if cpad is None else int(cpad)
    out = np.zeros((R, S, cpad), dtype=np.int8)
    out[..., :C] = np.transpose(_np(w)[:, 0], (1, 2, 0)).astype(np.int8)
    return torch.from_numpy(out)


def dwconv2d_i8_resident(xq, wq, qbias, stride, padding, rs, ob, relu):
    C = qbias.numel()
    x = np.ascontiguousarray(np.moveaxis(_np(xq).astype(np.int32), -1, 1)[:, :C])                  # NCHW, real channels
    w = np.ascontiguousarray(np.transpose(_np(wq).astype(np.int32), (2, 0, 1))[:C, None])           # [C, 1, R, S]
    acc = orc.conv2d_int(x, w, tuple(stride), tuple(padding), (1, 1), groups=C)
    y = _tail(acc, qbias, _shifts(rs, C), ob)
    if relu:
        y = np.maximum(y, np.float32(0))
    return native_doubles._to_i8_nhwc(y, ob, xq.shape[-1])


def recon_epilogue(acc, qbias, rs, ob, bitwidth=8, out=None):
    """The fused tail of the reference-shaped form (what a grouped convolution runs without the depthwise switch)."""
    assert bitwidth == 8
    return torch.from_numpy(_tail(_np(acc), qbias, _shifts(rs, acc.shape[1]), ob))


_DOUBLES = dict(pack_weight_dw=pack_weight_dw, dwconv2d_i8_resident=dwconv2d_i8_resident, recon_epilogue=recon_epilogue)


@contextlib.contextmanager
def installed():
    """native_doubles.installed() plus the doubles above.  _native.dwconv_supported stays the library's own: it is host
    arithmetic (fq_dwconv2d_i8_supported) and needs no GPU.  (The dense doubles of native_doubles take per-tensor shifts only:
    the CPU tests give per-channel bits to the depthwise layers alone, depthwise_nets.fixed_info(per_channel="depthwise").)"""
    with native_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
