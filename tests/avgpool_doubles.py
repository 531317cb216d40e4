"""Oracle-backed double for the windowed average-pool entry point of common.quantity._native (avgpool_i8_nhwc), on top of
tests/concat_doubles.py -- so that the CPU suite can run resident.enable(..., concat=True, avgpool=True) on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double follows the reference's chain literally:
DeQuantity of the source (real channels only) -> nn.AvgPool2d -> nn.ReLU -> Quantity at the consumer's bit.  Only shift = bit - grid
is an argument of the entry point (a power of two moves through the fp32 division unchanged), so the double takes the grid 0 and
the bit `shift`.
"""
import contextlib

import torch
from torch import nn

import concat_doubles
import native_doubles

GRID = 0


def avgpool_i8_nhwc(q, channels, kernel, stride, padding, count_include_pad, shift, relu, out=None):
    C = int(channels)
    f = torch.from_numpy(native_doubles._deq(q, GRID, C)).permute(0, 3, 1, 2).contiguous()          # [N, C, H, W] fp32
    pool = nn.AvgPool2d(tuple(kernel), tuple(stride), tuple(padding), ceil_mode=False, count_include_pad=bool(count_include_pad))
    y = pool(f)
    if relu:
        y = torch.relu(y)
    got = native_doubles._to_i8_nhwc(y.numpy(), GRID + int(shift), q.shape[-1])
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(avgpool_i8_nhwc=avgpool_i8_nhwc)


@contextlib.contextmanager
def installed():
    """concat_doubles.installed() plus the double above.  _native.avgpool_supported stays the library's own: it is host
    arithmetic (fq_avgpool_i8_nhwc_supported) and needs no GPU."""
    with concat_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
