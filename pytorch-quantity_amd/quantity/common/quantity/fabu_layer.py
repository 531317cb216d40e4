"""Marker layers: arithmetic that a model would normally write inline (``a + b``, ``torch.cat``,
``flatten``) exposed as ``nn.Module`` objects, so that forward hooks can see them by name.

Drop-in for reference quantity/common/quantity/fabu_layer.py (Eltwise :5-11, Concat :14-20,
Identity :23-29, View :31-36): same class names, constructor and forward signatures, so pickled
models and model definitions written against the reference import unchanged.  `Slice` is this
project's own (the reference has none): the channel split of a ShuffleNetV2 unit as a module.  These layers do no
quantisation work themselves; `tools.Reconstruction` swaps Eltwise for `NewAdd`.
"""
import torch
from torch import nn

__all__ = ["Eltwise", "Concat", "Identity", "View", "Slice"]


class _Marker(nn.Module):
    """Parameter-free module; exists only so that hooks and named_modules() can find the op."""

    def extra_repr(self):
        return "marker"


class Eltwise(_Marker):
    """Element-wise sum of two feature maps (the residual add of a ResNet block)."""

    def forward(self, x, y):
        return torch.add(x, y)


class Concat(_Marker):
    """Concatenation of two feature maps, channel axis by default."""

    def forward(self, x, y, dim=1):
        return torch.cat([x, y], dim)


class Identity(_Marker):
    """Pass-through; what a folded BatchNorm is replaced with (see utils.merge_bn)."""

    def forward(self, x):
        return x


class View(_Marker):
    """Flatten everything after the batch axis into a fresh tensor (the hook needs a new tensor,
    not an alias of the pooling output)."""

    def forward(self, x):
        return x.reshape(x.shape[0], -1).clone()


class Slice(_Marker):
    """Channels [start, stop) of a feature map as a fresh tensor (the channel split at the head of a
    ShuffleNetV2 unit; a bare ``x[:, a:b]`` is invisible to hooks and an alias of its source)."""

    def __init__(self, start, stop):
        super(Slice, self).__init__()
        self.start, self.stop = start, stop

    def forward(self, x):
        return x[:, self.start:self.stop].clone()

    def extra_repr(self):
        return "marker, channels [%s, %s)" % (self.start, self.stop)
