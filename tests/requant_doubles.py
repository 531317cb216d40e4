"""Oracle-backed double for the re-quantising concatenation (common.quantity._native.concat_rq_i8_nhwc), on top of every other
double -- so that the CPU suite can run resident.enable(..., concat=True, requant=True), alone or with all the other switches, on a
box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double takes the reference's chain literally, on
the CPU: the oracle's DeQuantity of every source at its own grid -> nearest upsampling (repeat) -> torch.cat -> ReLU -> the oracle's
Quantity at the consumer bit; the padding channels zero.  It does NOT use the closed form of tests/requant_ref.py:
test_requant_plan_cpu.py compares the two.  `calls` records [(channels, dtype bytes, up, relu, shift), ...] per launch.
"""
import contextlib

import numpy as np
import torch

import bilinear_doubles
import native_doubles
from oracle import fq_oracle as orc

calls = []


def literal_chain(srcs, bit):
    """srcs = [(int8 / int16 numpy [N, H / up, W / up, >= C] on grid g, C, up, relu, g)] -> int8 numpy [N, H, W, sum C] at `bit`, by the
    reference's ops one after another.  (A ReLU on one source alone is a ReLU in front of torch.cat; one on all is the ReLU behind.)"""
    parts = []
    for a, C, up, relu, g in srcs:
        v = orc.dequantity(np.ascontiguousarray(a[..., :C].transpose(0, 3, 1, 2)).astype(np.float32), int(g))
        t = torch.from_numpy(v)
        if up > 1:
            t = torch.repeat_interleave(torch.repeat_interleave(t, int(up), dim=2), int(up), dim=3)
        parts.append(torch.relu(t) if relu else t)
    cat = torch.cat(parts, 1)
    q = orc.quantity(np.ascontiguousarray(cat.numpy().astype(np.float32)), int(bit))
    return q.astype(np.int8).transpose(0, 2, 3, 1)


def concat_rq_i8_nhwc(srcs, out=None):
    assert 1 <= len(srcs) <= 8
    rows, total = [], 0
    for q, C, up, relu, shift in srcs:
        assert q.dtype in (torch.int8, torch.int16) and q.dim() == 4 and q.shape[3] == native_doubles.pad16(C) and up in (1, 2, 4)
        assert abs(int(shift)) <= 8
        rows.append((native_doubles._np(q), int(C), int(up), bool(relu), -int(shift)))      # (grid -shift, bit 0: the chain depends on b - g alone)
        total += int(C)
    calls.append([(C, a.dtype.itemsize, up, relu, -g) for a, C, up, relu, g in rows])
    body = literal_chain(rows, 0)
    y = np.zeros(body.shape[:3] + (native_doubles.pad16(total),), dtype=np.int8)
    y[..., :total] = body
    got = torch.from_numpy(y)
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(concat_rq_i8_nhwc=concat_rq_i8_nhwc)


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
    """bilinear_doubles.installed() -- all_doubles and the bilinear double -- plus the double above.  _native.concat_rq_supported
    stays the library's own: host arithmetic."""
    return _on(bilinear_doubles.installed)


def installed_all():
    """bilinear_doubles.installed_all() plus the double above: what enable() with all twelve switches needs."""
    return _on(bilinear_doubles.installed_all)
