"""The one cache of packed weights on an integer layer (_IntegerSimLayer._packed): the four packers are torch code that runs on
the host without the HIP library, so every slot is checked here."""
import pickle

import pytest
import torch
from torch import nn


def _layer(conv):
    from common.quantity import NewConv2d
    return NewConv2d(conv, {"weight_bit": 5, "bias_bit": 4, "input_bit": 4, "output_bit": 4})


def _cases():
    from common.quantity import new_quantity_op as ops
    return {"dense": ("_w_i8", nn.Conv2d(8, 8, 3, padding=1), ops._pack_dense, (8, 3, 3, 16)),
            "folded_stem": ("_w_i8", nn.Conv2d(3, 8, 3, padding=1), ops._pack_dense, (8, 3, 1, 16)),
            "stem": ("_w_stem", nn.Conv2d(3, 8, 3, padding=1), ops._pack_stem, (3, 64, 32)),
            "depthwise": ("_w_dw", nn.Conv2d(8, 8, 3, padding=1, groups=8), ops._pack_depthwise, (3, 3, 16)),
            "grouped": ("_w_gc", nn.Conv2d(8, 8, 3, padding=1, groups=2), ops._pack_grouped, (4, 9, 1, 4, 4))}


@pytest.mark.parametrize("case", ["dense", "folded_stem", "stem", "depthwise", "grouped"])
def test_packed_weights_are_cached_until_the_weight_changes_and_are_not_pickled(case):
    from common.quantity import new_quantity_op as ops
    slot, conv, pack, shape = _cases()[case]
    assert slot in ops._WEIGHT_SLOTS
    m = _layer(conv)
    assert slot not in m.__dict__
    first = m._packed(slot, conv, pack)
    assert first.dtype == torch.int8 and tuple(first.shape) == shape
    assert torch.equal(first, pack(conv)) and first.any()
    assert m._packed(slot, conv, pack) is first                         # a second call returns the same object
    assert m.__dict__[slot][1] is first and set(m.__dict__) & set(ops._WEIGHT_SLOTS) == {slot}
    with torch.no_grad():
        conv.weight.neg_()                                              # an in-place edit bumps the version: repacked
    second = m._packed(slot, conv, pack)
    assert second is not first and torch.equal(second, pack(conv)) and not torch.equal(second, first)
    assert m._packed(slot, conv, pack) is second
    again = pickle.loads(pickle.dumps(m))                               # derived data stays out of the pickle
    assert slot in m.__dict__ and not set(again.__dict__) & set(ops._WEIGHT_SLOTS)
    assert torch.equal(again._packed(slot, again.Conv, pack), second)
