"""Oracle-backed doubles of the integer producers with the trailing `clip=` keyword (common.quantity._native: conv2d_i8_resident,
conv2d_i8_stem, dwconv2d_i8_resident, gconv2d_i8_resident), on top of tests/grouped_doubles.py -- so that the CPU suite can run a
network with nn.ReLU6 modules with and without resident.enable(relu6=True).

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  A clipped double does NOT clamp integers.  It runs
the unclipped double of the module it wraps (the reference's fp32 chain up to DeQuantity), de-quantises its int8 result, applies
torch.nn.functional.relu6 in fp32 -- the reference's own module -- and quantises again at the output bit: what the next layer's
Quantity would read behind the fp32 ReLU6.  The Sp range it is given must be the one relu6_clip states for the layer's bit.
`calls` records (entry point, clip) of every producer launch, for the tests that compare call sequences.
"""
import contextlib

import numpy as np
import torch

import grouped_doubles
import native_doubles
from oracle import fq_oracle as orc

calls = []


def _requantised_relu6(q, ob, clip):
    from common.quantity import _native
    assert clip == _native.relu6_clip(ob) and clip[1] < 127, (clip, ob)      # (from 127 on the caller passes no clip at all)
    y = orc.dequantity(np.ascontiguousarray(native_doubles._np(q).astype(np.float32)), ob)
    y = torch.nn.functional.relu6(torch.from_numpy(y)).numpy()
    return torch.from_numpy(orc.quantity(np.ascontiguousarray(y), ob).astype(np.int8))


def _clipped(name, plain, ob_index, q_of=lambda out: out, with_q=lambda out, q: q):
    def double(*args, clip=None):
        calls.append((name, clip))
        if clip is None:
            return plain(*args)
        args = list(args)
        assert args[-1], "a clip replaces a fused ReLU: the planner passes relu=True with it"
        out = plain(*args[:-1], False)
        return with_q(out, _requantised_relu6(q_of(out), args[ob_index], clip))
    return double


def _dense(plain):
    def with_q(out, q):
        y = None
        if out[0] is not None:                                # the fp32 output, clipped by the reference's module
            y = torch.nn.functional.relu6(out[0])
        return y, q

    def double(xq, wq, qbias, stride, padding, dilation, rs, ob, want_f32, want_i8, relu, clip=None):
        calls.append(("conv2d_i8_resident", clip))
        if clip is None:
            return plain(xq, wq, qbias, stride, padding, dilation, rs, ob, want_f32, want_i8, relu)
        assert relu
        y, q = plain(xq, wq, qbias, stride, padding, dilation, rs, ob, want_f32, True, False)
        return with_q((y, q), _requantised_relu6(q, ob, clip) if want_i8 else None)
    return double


@contextlib.contextmanager
def installed():
    """grouped_doubles.installed() with the four producers wrapped to take `clip=`; relu6_clip stays the product's own."""
    with grouped_doubles.installed() as nat:
        wrapped = dict(conv2d_i8_resident=_dense(nat.conv2d_i8_resident),
                       conv2d_i8_stem=_clipped("conv2d_i8_stem", nat.conv2d_i8_stem, 9),
                       dwconv2d_i8_resident=_clipped("dwconv2d_i8_resident", nat.dwconv2d_i8_resident, 6),
                       gconv2d_i8_resident=_clipped("gconv2d_i8_resident", nat.gconv2d_i8_resident, 8))
        saved = {k: getattr(nat, k) for k in wrapped}
        for k, v in wrapped.items():
            setattr(nat, k, v)
        del calls[:]
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
