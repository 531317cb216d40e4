"""EDSR (Lim et al., "Enhanced Deep Residual Networks for Single Image Super-Resolution", 2017) in "fabu" style: the sub-pixel
super-resolution network whose upsampler is a convolution to r^2 * n_feats channels followed by nn.PixelShuffle(r).

  head       conv3x3(n_colors -> n_feats)
  body       n_resblocks residual blocks, Eltwise(conv3x3 -> ReLU -> conv3x3 (x), x) with NO ReLU behind the sum and no
             BatchNorm (the paper removes both), then conv3x3, then the global skip Eltwise(body, head)
  upsampler  scale 2 or 3: conv3x3(n_feats -> r^2 n_feats) -> nn.PixelShuffle(r); scale 4: two x2 stages
  tail       conv3x3(n_feats -> n_colors), linear: the image [N, n_colors, scale * H, scale * W]

Residual adds are modules (Eltwise) and the ReLUs are out of place, so forward hooks see each cared tensor and Quantity ->
Reconstruction.ReconModel take the model as it stands, with `PixelShuffle` in tools/configs.yml.  resident.enable(...,
pixelshuffle=True) runs every nn.PixelShuffle on fq_pixel_shuffle_i8_nhwc; without the switch the widest tensor of the network
leaves the integer domain there.  The paper's residual scaling (0.1, for the 256-feature model) and its mean shift are left out:
both are foreign elementwise code to the calibrator.

The reference ships no such model; this one is written from the architecture.  Any other scale raises ValueError.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise  # noqa: E402


class ResBlock(nn.Module):
    """Eltwise(conv -> ReLU -> conv (x), x)"""

    def __init__(self, n_feats):
        super(ResBlock, self).__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feats, n_feats, 3, 1, 1), nn.ReLU(False), nn.Conv2d(n_feats, n_feats, 3, 1, 1))
        self.Eltwise = Eltwise()

    def forward(self, x):
        return self.Eltwise(self.body(x), x)


class EDSR(nn.Module):

    def __init__(self, scale=2, n_resblocks=16, n_feats=64, n_colors=3):
        super(EDSR, self).__init__()
        if scale not in (2, 3, 4):
            raise ValueError("EDSR: scale must be 2, 3 or 4, got %r" % (scale,))
        if n_resblocks < 1 or n_feats < 1 or n_colors < 1:
            raise ValueError("EDSR: n_resblocks, n_feats and n_colors must be positive, got %r, %r, %r" % (n_resblocks, n_feats, n_colors))
        self.scale = scale
        self.head = nn.Conv2d(n_colors, n_feats, 3, 1, 1)
        self.blocks = nn.Sequential(*[ResBlock(n_feats) for _ in range(n_resblocks)])
        self.body_conv = nn.Conv2d(n_feats, n_feats, 3, 1, 1)
        self.Eltwise = Eltwise()
        stages = []
        for r in ((2, 2) if scale == 4 else (scale,)):
            stages += [nn.Conv2d(n_feats, r * r * n_feats, 3, 1, 1), nn.PixelShuffle(r)]
        self.upsampler = nn.Sequential(*stages)
        self.tail = nn.Conv2d(n_feats, n_colors, 3, 1, 1)

    def forward(self, x):
        x = self.head(x)
        x = self.Eltwise(self.body_conv(self.blocks(x)), x)
        return self.tail(self.upsampler(x))
