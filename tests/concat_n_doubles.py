"""Double for the N-source Concat entry point of common.quantity._native (concat_n_i8_nhwc), on top of tests/avgpool_doubles.py --
so that the CPU suite can run resident.enable(..., concat=True, flatten=True) on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double is the rule of include/fq.h
(fq_concat_n_i8_nhwc) in torch: with base_i = C_0 + ... + C_{i-1}, out[n][h][w][c] = f_i(src_i[n][h / up_i][w / up_i][c - base_i])
for base_i <= c < base_i + C_i, zero behind sum C, f_i = max(., 0) where relu_i is set.  Nearest upsampling of the integers is
torch's repeat_interleave on both axes; the reference's own chain (DeQuantity -> F.interpolate -> ReLU -> torch.cat -> Quantity on
the grid 0) is asserted to give the same integers.
"""
import contextlib

import torch
import torch.nn.functional as F

import avgpool_doubles
import native_doubles


def concat_n_rule(srcs):
    """srcs = [(int8 [N, h, w, Cpad] tensor, C, up, relu), ...] -> int8 [N, H, W, pad16(sum C)]"""
    parts = []
    for q, C, up, relu in srcs:
        a = q[..., :int(C)]
        if int(up) != 1:
            a = a.repeat_interleave(int(up), dim=1).repeat_interleave(int(up), dim=2)
        parts.append(torch.clamp(a, min=0) if relu else a)
    y = torch.cat(parts, dim=3)
    total = y.shape[3]
    out = torch.zeros(tuple(y.shape[:3]) + (native_doubles.pad16(total),), dtype=torch.int8)
    out[..., :total] = y
    return out


def concat_n_i8_nhwc(srcs, out=None):
    assert 1 <= len(srcs) <= 8, "fq_concat_n_i8_nhwc takes one to eight sources"
    got = concat_n_rule([(q.cpu(), C, up, relu) for q, C, up, relu in srcs])
    chain = []
    for q, C, up, relu in srcs:                             # the reference's chain on the grid 0
        f = q[..., :int(C)].float().permute(0, 3, 1, 2).contiguous()
        if int(up) != 1:
            f = F.interpolate(f, scale_factor=float(up), mode="nearest")
        chain.append(torch.relu(f) if relu else f)
    ref = torch.cat(chain, 1).permute(0, 2, 3, 1)
    assert torch.equal(got[..., :ref.shape[3]].float(), ref) and not got[..., ref.shape[3]:].any()
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(concat_n_i8_nhwc=concat_n_i8_nhwc)


@contextlib.contextmanager
def installed():
    """avgpool_doubles.installed() (which holds the Concat and the native doubles) plus the double above.
    _native.concat_n_supported stays the library's own: it is host arithmetic and needs no GPU."""
    with avgpool_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
