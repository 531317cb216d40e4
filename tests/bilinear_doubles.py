"""Oracle-backed double for the resident int8 bilinear upsampling (common.quantity._native.upsample_bilinear_i8_nhwc), on top of
every other double -- so that the CPU suite can run resident.enable(..., concat=True, bilinear=True), alone or with all the other
switches, on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double takes the reference's chain literally, on
the CPU: the oracle's DeQuantity at the source grid -> torch's own F.interpolate(mode="bilinear", align_corners=False) on the fp32
NCHW tensor -> ReLU -> the oracle's Quantity at the consumer bit; the padding channels zero.  It does NOT use the closed form of
tests/bilinear_ref.py: test_bilinear_plan_cpu.py compares the two.  `calls` records (channels, source shape, up, shift, relu).
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import all_doubles
import native_doubles
import topdown_doubles
from oracle import fq_oracle as orc

calls = []


def literal_chain(x, c, up, grid, bit, relu):
    """x int8 numpy [N, H, W, >= c] on `grid` -> int8 numpy [N, up H, up W, c] at `bit`, by the reference's ops one after another."""
    v = orc.dequantity(np.ascontiguousarray(x[..., :c].transpose(0, 3, 1, 2)).astype(np.float32), int(grid))
    with torch.no_grad():
        t = F.interpolate(torch.from_numpy(v), scale_factor=float(up), mode="bilinear", align_corners=False)
        if relu:
            t = torch.relu(t)
    q = orc.quantity(np.ascontiguousarray(t.numpy().astype(np.float32)), int(bit))
    return q.astype(np.int8).transpose(0, 2, 3, 1)


def upsample_bilinear_i8_nhwc(q, channels, up, shift, relu, out=None):
    c, up, shift = int(channels), int(up), int(shift)
    assert q.dtype == torch.int8 and q.dim() == 4 and q.shape[3] == native_doubles.pad16(c) and up in (2, 4) and abs(shift) <= 8
    calls.append((c, tuple(q.shape), up, shift, bool(relu)))
    x = native_doubles._np(q)
    y = np.zeros((x.shape[0], up * x.shape[1], up * x.shape[2], x.shape[3]), dtype=np.int8)
    y[..., :c] = literal_chain(x, c, up, 0, shift, relu)     # (the chain depends on bit - grid alone: every step scales by a power of two)
    got = torch.from_numpy(y)
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(upsample_bilinear_i8_nhwc=upsample_bilinear_i8_nhwc)


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
    """all_doubles.installed() plus the double above.  _native.upsample_bilinear_supported stays the library's own: host arithmetic."""
    return _on(all_doubles.installed)


def installed_all():
    """topdown_doubles.installed() -- all_doubles, the int16 pool and the add with an upsampled operand -- plus the double above:
    what enable() with all eleven switches needs."""
    return _on(topdown_doubles.installed)
