"""Oracle-backed double for the pixel shuffle / unshuffle entry point (common.quantity._native.pixel_shuffle_i8_nhwc), on top of every
other double -- so that the CPU suite can run resident.enable(..., pixelshuffle=True), alone or with all the other switches, on a
box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double is the index rule of include/fq.h written
in numpy (pixelshuffle_nets.pixel_rule), and it checks itself against the reference's chain on the CPU: the oracle's DeQuantity of
the real channels -> torch's own pixel_shuffle / pixel_unshuffle -> the oracle's Quantity at the same grid gives the same integers
(the grid is not an argument of the entry point; the double uses 0 and asserts that the round trip is exact).  `calls` records
(C, r, inverse, shape of the source) of every launch.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import native_doubles
import pixelshuffle_nets
import requant_doubles
from oracle import fq_oracle as orc

GRID = 0
calls = []


def pixel_shuffle_i8_nhwc(x, C, r, inverse, out=None):
    C, r, inverse = int(C), int(r), int(bool(inverse))
    assert x.dtype == torch.int8 and x.dim() == 4 and r in (2, 3, 4) and C >= 1
    real = C if inverse else C * r * r
    assert x.shape[3] == native_doubles.pad16(real)
    calls.append((C, r, inverse, tuple(x.shape)))
    got = torch.from_numpy(pixelshuffle_nets.pixel_rule(native_doubles._np(x), C, r, inverse))
    # the reference's chain on the fp32 form
    f = torch.from_numpy(native_doubles._deq(x, GRID, real)).permute(0, 3, 1, 2).contiguous()
    f = F.pixel_unshuffle(f, r) if inverse else F.pixel_shuffle(f, r)
    out_c = C * r * r if inverse else C
    want = native_doubles._to_i8_nhwc(f.numpy(), GRID, native_doubles.pad16(out_c))
    assert torch.equal(got, want)
    assert np.array_equal(orc.dequantity(got[..., :out_c].numpy().astype(np.float32), GRID), f.permute(0, 2, 3, 1).numpy())
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(pixel_shuffle_i8_nhwc=pixel_shuffle_i8_nhwc)


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
    """requant_doubles.installed() -- all_doubles, the bilinear and the re-quantising Concat double -- plus the double above.
    _native.pixel_shuffle_supported stays the library's own: host arithmetic."""
    return _on(requant_doubles.installed)


def installed_all():
    """requant_doubles.installed_all() plus the double above: what enable() with all thirteen switches needs."""
    return _on(requant_doubles.installed_all)
