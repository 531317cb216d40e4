"""Oracle-backed double for the resident add with a nearest-upsampled operand (common.quantity._native.add_up_resident), on top of
every other double -- so that the CPU suite can run resident.enable(..., concat=True, topdown=True), alone or with all the other
switches, on a box without a GPU.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double says what the rule of include/fq.h says:
the coarse operand repeated `up` times along H and W (torch.repeat_interleave: what nn.Upsample(mode="nearest") does to values),
then the existing add double, which follows the reference's chain DeQuantity -> add -> Sp -> ReLU -> Quantity literally.
"""
import contextlib

import torch

import native_doubles
import sum_pool_doubles


def add_up_resident(x, gx, y, gy, up, want_wide, g_wide, want_narrow, ib, relu):
    assert x.dtype in (torch.int8, torch.int16) and y.dtype in (torch.int8, torch.int16) and up in (2, 4)
    big = torch.repeat_interleave(torch.repeat_interleave(y, up, dim=1), up, dim=2)
    assert tuple(big.shape) == tuple(x.shape), (tuple(x.shape), tuple(y.shape), up)
    return native_doubles.add_resident(x, gx, big, gy, want_wide, g_wide, want_narrow, ib, relu)


_DOUBLES = dict(add_up_resident=add_up_resident)


@contextlib.contextmanager
def installed():
    """sum_pool_doubles.installed_all() -- all_doubles.installed() and the int16 pool -- plus the double above.
    _native.add_up_supported stays the library's own: it is host arithmetic (fq_add_up_resident_supported) and needs no GPU."""
    with sum_pool_doubles.installed_all() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
