"""Oracle-backed double for the transposed-convolution entry point (common.quantity._native.deconv2d_i8_resident), on top of every
other double (pixelshuffle_doubles, which stacks on requant_doubles and all_doubles) -- so that the CPU suite can run
resident.enable(..., deconv=True), alone or with all the other switches, on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double follows the reference-shaped chain
literally: the integers of the real input channels -> torch's own conv_transpose2d in float64 with the weights read back out of
the pack (deconv_nets.unpack_rule) -> the oracle's RightShift + BiasAdd + Sp + DeQuantity (recon_epilogue) -> nn.ReLU -> the next
layer's Quantity(ob).  It checks itself against the kernel's own numpy form, the phase-by-phase integer rule (deconv_nets.phase_acc).
A clip (a fused nn.ReLU6) goes through relu6_doubles' fp32 ReLU6.  _native.pack_weight_deconv and deconv_supported stay the
product's own: torch ops and host arithmetic.  `calls` records (C, K, kernel, stride, padding, output_padding, relu, clip, shape of
the source) of every launch.
"""
import contextlib

import numpy as np
import torch

import deconv_nets
import native_doubles
import pixelshuffle_doubles
import relu6_doubles
from oracle import fq_oracle as orc

calls = []


def deconv2d_i8_resident(xq, wq, qbias, C, kernel, stride, padding, output_padding, rs, ob, relu, clip=None, out=None):
    C, K = int(C), qbias.numel()
    kernel, stride, padding, output_padding = (tuple(int(v) for v in t) for t in (kernel, stride, padding, output_padding))
    assert xq.dtype == torch.int8 and xq.dim() == 4 and xq.shape[3] == native_doubles.pad16(C) and isinstance(rs, int)
    calls.append((C, K, kernel, stride, padding, output_padding, bool(relu), clip, tuple(xq.shape)))
    c = deconv_nets.case(xq.shape[0], xq.shape[1], xq.shape[2], C, K, kernel, stride, padding, output_padding, rs=rs)
    x = native_doubles._np(xq)
    w = deconv_nets.unpack_rule(native_doubles._np(wq), c)
    acc = deconv_nets.f64_acc(x, w, c)                                                    # [N, P, Q, K]
    assert np.array_equal(acc, deconv_nets.phase_acc(x, native_doubles._np(wq), c))      # the kernel's form: phase by phase
    assert np.abs(acc).max(initial=0) < 2 ** 24
    y = orc.recon_epilogue(np.ascontiguousarray(np.moveaxis(acc, -1, 1), dtype=np.float32), native_doubles._np(qbias).astype(np.float32),
                           rs, ob)
    if clip is not None:
        assert relu, "a clip replaces a fused ReLU: the planner passes relu=True with it"
        q = relu6_doubles._requantised_relu6(native_doubles._to_i8_nhwc(y, ob, native_doubles.pad16(K)), ob, clip)
    else:
        if relu:
            y = np.maximum(y, np.float32(0))
        q = native_doubles._to_i8_nhwc(y, ob, native_doubles.pad16(K))
    if out is not None:
        out.copy_(q)
        return out
    return q


_DOUBLES = dict(deconv2d_i8_resident=deconv2d_i8_resident)


@contextlib.contextmanager
def _on(base):
    with base() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        del calls[:]
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)


def installed():
    """pixelshuffle_doubles.installed() -- all_doubles and everything stacked on it since -- plus the double above."""
    return _on(pixelshuffle_doubles.installed)


def installed_all():
    """pixelshuffle_doubles.installed_all() plus the double above: what enable() with all fourteen switches needs."""
    return _on(pixelshuffle_doubles.installed_all)
