"""Oracle-backed double for the Concat / nearest-upsampling entry point of common.quantity._native (concat_i8_nhwc), on top of
tests/native_doubles.py -- so that the CPU suite can run resident.enable(..., concat=True) on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double follows the reference's chain literally:
DeQuantity of every operand (real channels only) -> F.interpolate(mode="nearest") -> torch.cat along the channels -> nn.ReLU ->
Quantity at the operands' grid.  The grid is not an argument of the entry point (the integers do not depend on it): any grid
gives the same integers back, the double uses 0 and asserts that the round trip is exact.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import native_doubles
from oracle import fq_oracle as orc

GRID = 0


def concat_i8_nhwc(srcs, relu, out=None):
    parts = []
    for q, C, up in srcs:
        f = torch.from_numpy(native_doubles._deq(q, GRID, int(C)))                  # [N, h, w, C] fp32
        f = f.permute(0, 3, 1, 2).contiguous()
        if int(up) != 1:
            f = F.interpolate(f, scale_factor=float(up), mode="nearest")
        parts.append(f)
    y = torch.cat(parts, 1)
    if relu:
        y = torch.relu(y)
    total = y.shape[1]
    got = native_doubles._to_i8_nhwc(y.numpy(), GRID, native_doubles.pad16(total))
    assert np.array_equal(orc.dequantity(got[..., :total].numpy().astype(np.float32), GRID), y.permute(0, 2, 3, 1).numpy())
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(concat_i8_nhwc=concat_i8_nhwc)


@contextlib.contextmanager
def installed():
    """native_doubles.installed() plus the double above.  _native.concat_supported stays the library's own: it is host
    arithmetic (fq_concat_i8_nhwc_supported) and needs no GPU."""
    with native_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
