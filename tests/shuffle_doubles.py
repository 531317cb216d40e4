"""Oracle-backed doubles for a ShuffleNetV2-style network on a box without a GPU: the depthwise and native doubles
(tests/depthwise_doubles.py), the Concat double (tests/concat_doubles.py) and a double of the channel shuffle / slice entry point
of common.quantity._native (shuffle_i8_nhwc) -- so that the CPU suite can run resident.enable(..., depthwise=True, concat=True,
shuffle=True).

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The double is the index rule of include/fq.h written
in numpy (shuffle_nets.shuffle_rule), and it checks itself against the reference's chain: DeQuantity of the real channels ->
x[:, c_off:c_off + c] -> torch.channel_shuffle -> Quantity at the same grid gives the same integers (the grid is not an argument
of the entry point; the double uses 0 and asserts that the round trip is exact).  `calls` records (c_in, c_off, c, groups, shape
of the source) of every launch.
"""
import contextlib

import numpy as np
import torch

import concat_doubles
import depthwise_doubles
import native_doubles
import shuffle_nets
from oracle import fq_oracle as orc

GRID = 0
calls = []


def shuffle_i8_nhwc(x_q, c_in, c_off, c, groups, out=None):
    c_in, c_off, c, groups = int(c_in), int(c_off), int(c), int(groups)
    assert x_q.dtype == torch.int8 and x_q.dim() == 4 and x_q.shape[3] == native_doubles.pad16(c_in)
    assert 0 <= c_off and c >= 1 and c_off + c <= c_in and groups >= 1 and c % groups == 0
    calls.append((c_in, c_off, c, groups, tuple(x_q.shape)))
    got = torch.from_numpy(shuffle_nets.shuffle_rule(native_doubles._np(x_q), c_off, c, groups))
    # the reference's chain on the fp32 form
    f = torch.from_numpy(native_doubles._deq(x_q, GRID, c_in)).permute(0, 3, 1, 2).contiguous()
    f = torch.channel_shuffle(f[:, c_off:c_off + c].clone(), groups)
    want = native_doubles._to_i8_nhwc(f.numpy(), GRID, native_doubles.pad16(c))
    assert torch.equal(got, want)
    assert np.array_equal(orc.dequantity(got[..., :c].numpy().astype(np.float32), GRID), f.permute(0, 2, 3, 1).numpy())
    if out is not None:
        out.copy_(got)
        return out
    return got


_DOUBLES = dict(shuffle_i8_nhwc=shuffle_i8_nhwc, concat_i8_nhwc=concat_doubles.concat_i8_nhwc)


@contextlib.contextmanager
def installed():
    """depthwise_doubles.installed() plus the Concat double and the double above.  _native.shuffle_supported stays the
    library's own: it is host arithmetic (fq_shuffle_i8_nhwc_supported) and needs no GPU."""
    with depthwise_doubles.installed() as nat:
        saved = {k: getattr(nat, k) for k in _DOUBLES}
        for k, v in _DOUBLES.items():
            setattr(nat, k, v)
        del calls[:]
        try:
            yield nat
        finally:
            for k, v in saved.items():
                setattr(nat, k, v)
