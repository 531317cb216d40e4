"""A YOLOv4-tiny-shaped detector backbone, neck and heads in "fabu" style: two 3x3 stride-2 stem convolutions, three CSP blocks, a
3x3 convolution, and a two-scale neck with two linear 1x1 heads.  Every convolution but the heads is conv -> BN ->
nn.LeakyReLU(0.1).

  CSP block (c)   x = conv3x3(c -> c); r = Slice(c/2, c)(x); a = conv3x3(c/2 -> c/2)(r); b = conv3x3(c/2 -> c/2)(a);
                  m = conv1x1(c -> c)(Concat(b, a)); y = MaxPool2d(2)(Concat(x, m))           (2c channels out; m is the route)
  neck            n = conv1x1(512 -> 256); coarse head: conv3x3(256 -> 512) -> 1x1 linear;
                  fine head: conv1x1(256 -> 128)(n) -> nearest upsampling x2 -> Concat with the last block's route m ->
                  conv3x3(384 -> 256) -> 1x1 linear

The split, the joins and the upsampling are modules (Slice, Concat, nn.UpsamplingNearest2d -- the type name tools/configs.yml
lists; nn.Upsample(scale_factor=2) computes the same but graph discovery goes by type name), and every activation is an
out-of-place nn.LeakyReLU, so forward hooks see each cared tensor and merge_bn -> Quantity -> Reconstruction.ReconModel take the
model as it stands (tools/configs.yml lists LeakyReLU among the traced op types).  resident.enable(..., concat=True, shuffle=True,
activations=True) keeps the network between the stem and the heads in int8: each LeakyReLU is a 256-entry table
(fq_act_lut_i8_nhwc).

`heads=2` returns (coarse, fine); `heads=1` ends the model in the fine head alone (the coarse head is not built), for flows that
take one output.  The reference ships no YOLO; this one is written from the architecture (Bochkovskiy et al. 2020, the tiny
configuration).  `width` is the first stem convolution's (32 in the paper; tests build a narrow network), `num_outputs` the
channels of a head (anchors x (5 + classes)), `batch_norm=False` builds the network as merge_bn leaves it.  The input side must be
a multiple of 32.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, Slice  # noqa: E402


def _cbl(cin, cout, k, stride=1, batch_norm=True):
    layers = [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=not batch_norm)]
    if batch_norm:
        layers.append(nn.BatchNorm2d(cout))
    return nn.Sequential(*layers, nn.LeakyReLU(0.1))


class CSPBlock(nn.Module):

    def __init__(self, c, batch_norm=True):
        super(CSPBlock, self).__init__()
        self.conv = _cbl(c, c, 3, batch_norm=batch_norm)
        self.right = Slice(c // 2, c)
        self.conv_a = _cbl(c // 2, c // 2, 3, batch_norm=batch_norm)
        self.conv_b = _cbl(c // 2, c // 2, 3, batch_norm=batch_norm)
        self.Concat_inner = Concat()
        self.route = _cbl(c, c, 1, batch_norm=batch_norm)
        self.Concat_outer = Concat()
        self.pool = nn.MaxPool2d(2)

    def forward(self, x):
        x = self.conv(x)
        a = self.conv_a(self.right(x))
        m = self.route(self.Concat_inner(self.conv_b(a), a))
        return self.pool(self.Concat_outer(x, m)), m


class YoloTiny(nn.Module):

    def __init__(self, num_outputs=255, width=32, heads=2, batch_norm=True):
        super(YoloTiny, self).__init__()
        assert heads in (1, 2) and width % 4 == 0
        w = width
        self.stem1 = _cbl(3, w, 3, 2, batch_norm)
        self.stem2 = _cbl(w, 2 * w, 3, 2, batch_norm)
        self.block1, self.block2, self.block3 = (CSPBlock(2 * w, batch_norm), CSPBlock(4 * w, batch_norm),
                                                 CSPBlock(8 * w, batch_norm))
        self.conv = _cbl(16 * w, 16 * w, 3, batch_norm=batch_norm)
        self.neck = _cbl(16 * w, 8 * w, 1, batch_norm=batch_norm)
        self.heads = heads
        if heads == 2:
            self.coarse = _cbl(8 * w, 16 * w, 3, batch_norm=batch_norm)
            self.coarse_head = nn.Conv2d(16 * w, num_outputs, 1)
        self.lateral = _cbl(8 * w, 4 * w, 1, batch_norm=batch_norm)
        self.up = nn.UpsamplingNearest2d(scale_factor=2)
        self.Concat = Concat()
        self.fine = _cbl(12 * w, 8 * w, 3, batch_norm=batch_norm)
        self.fine_head = nn.Conv2d(8 * w, num_outputs, 1)

    def forward(self, x):
        x, _ = self.block1(self.stem2(self.stem1(x)))
        x, _ = self.block2(x)
        x, route = self.block3(x)
        n = self.neck(self.conv(x))
        fine = self.fine_head(self.fine(self.Concat(self.up(self.lateral(n)), route)))
        if self.heads == 1:
            return fine
        return self.coarse_head(self.coarse(n)), fine
