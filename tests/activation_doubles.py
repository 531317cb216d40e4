"""Oracle-backed doubles for a network with table activations on a box without a GPU: everything of tests/shuffle_doubles.py
(depthwise, native, Concat, shuffle / slice) plus doubles of the two new entry points of common.quantity._native, act_lut_i8_nhwc
and build_act_table -- so that the CPU suite can run resident.enable(..., concat=True, shuffle=True, activations=True).

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The kernel's double is its rule in numpy
(activation_nets.act_lut_rule: table lookup plus zeroed padding).  build_act_table's double follows the product's recipe with the
oracle's DeQuantity and Quantity around the module's own forward on a CPU tensor.  `calls` records (channels, shape) per launch.
"""
import contextlib

import numpy as np
import torch

import activation_nets as an
import native_doubles
import shuffle_doubles
from oracle import fq_oracle as orc

calls = []


def act_lut_i8_nhwc(x_q, c, table, out=None):
    c = int(c)
    assert x_q.dtype == torch.int8 and x_q.dim() == 4 and x_q.shape[3] == native_doubles.pad16(c)
    assert table.dtype == torch.int8 and table.numel() == 256
    calls.append((c, tuple(x_q.shape)))
    got = torch.from_numpy(an.act_lut_rule(native_doubles._np(x_q), c, native_doubles._np(table)))
    if out is not None:
        out.copy_(got)
        return out
    return got


def build_act_table(module, grid, bit):
    with torch.no_grad():
        q = np.arange(-128, 128, dtype=np.float32).reshape(1, 1, 16, 16)
        x = torch.from_numpy(orc.dequantity(q, int(grid)))
        y = type(module).forward(module, x)
        return torch.from_numpy(orc.quantity(y.contiguous().numpy().astype(np.float32), int(bit))).reshape(256).to(torch.int8)


def elementwise_table(module, grid, bit):
    """The same 256 entries one at a time: DeQuantity -> module -> Quantity on a single-element tensor per integer."""
    out = np.zeros(256, dtype=np.int8)
    with torch.no_grad():
        for q in range(-128, 128):
            x = torch.from_numpy(orc.dequantity(np.full((1, 1, 1, 1), q, dtype=np.float32), int(grid)))
            y = type(module).forward(module, x)
            out[q + 128] = orc.quantity(y.numpy().astype(np.float32), int(bit)).reshape(())
    return out


_DOUBLES = dict(act_lut_i8_nhwc=act_lut_i8_nhwc, build_act_table=build_act_table)


@contextlib.contextmanager
def installed():
    """shuffle_doubles.installed() plus the two doubles above.  _native.act_lut_supported stays the library's own: host arithmetic."""
    with shuffle_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        del calls[:]
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
