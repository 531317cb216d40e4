"""Oracle-backed double for the windowed average pool over a NewAdd sum (common.quantity._native.avgpool_i16_nhwc), on top of
tests/avgpool_doubles.py -- so that the CPU suite can run resident.enable(..., avgpool=True, sums=True) on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double follows the reference's chain literally:
DeQuantity of the int16 source (real channels only) -> nn.AvgPool2d -> nn.ReLU -> Quantity at the consumer's bit.  Only
shift = bit - grid is an argument of the entry point (a power of two moves through the fp32 division unchanged), so the double
takes the grid 0 and the bit `shift`, as the int8 double does.
"""
import contextlib

import torch

import all_doubles
import avgpool_doubles


def avgpool_i16_nhwc(q16, channels, kernel, stride, padding, count_include_pad, shift, relu, out=None):
    assert q16.dtype == torch.int16, q16.dtype
    return avgpool_doubles.avgpool_i8_nhwc(q16, channels, kernel, stride, padding, count_include_pad, shift, relu, out)


_DOUBLES = dict(avgpool_i16_nhwc=avgpool_i16_nhwc)


@contextlib.contextmanager
def _over(base):
    with base.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)


def installed():
    """avgpool_doubles.installed() plus the double above.  _native.avgpool_i16_supported stays the library's own: it is host
    arithmetic (fq_avgpool_i16_nhwc_supported) and needs no GPU."""
    return _over(avgpool_doubles)


def installed_all():
    """all_doubles.installed() (every switch of resident.enable()) plus the double above."""
    return _over(all_doubles)
