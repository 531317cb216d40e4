"""A U-Net with a bilinear decoder in "fabu" style (Ronneberger et al. 2015; the bilinear variant that replaces the transposed
convolutions by nn.Upsample and halves the decoder's widths, so that a level's Concat has as many channels as the level below).

  level (cin -> c)   conv3x3(cin -> c) -> [BN] -> ReLU -> conv3x3(c -> c) -> [BN] -> ReLU
  encoder            level(3 -> w), then `depth` times nn.MaxPool2d(2) -> level; widths w, 2w, 4w, ..., the lowest level keeps the
                     width of the one above it (w * 2^(depth-1))
  decoder            `depth` times: nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) -> Concat(skip, up) ->
                     level(2c -> c / 2) (the last one: 2w -> w)
  head               conv1x1(w -> num_classes), linear: a dense map [N, num_classes, input_size, input_size]

The pools, the upsamplings and the joins are modules (nn.MaxPool2d, nn.Upsample -- the type name tools/configs.yml lists --,
Concat) and every ReLU is out of place, so forward hooks see each cared tensor and merge_bn -> Quantity ->
Reconstruction.ReconModel take the model as it stands.  resident.enable(..., concat=True, bilinear=True) keeps the whole network
between the image and the head in int8: each upsampling is one launch of fq_upsample_bilinear_i8_nhwc.  Without `bilinear` every
decoder level leaves the integer domain twice (the convolution in front of the upsampling writes fp32, the Concat behind it is
foreign code).

`up="deconv"` builds the paper's own decoder instead: the widths double down to the lowest level (w * 2^depth) and a decoder step
is nn.ConvTranspose2d(2c -> c, up_kernel, stride=2) -> Concat(skip, up) -> level(2c -> c).  `up_kernel` 2 is the paper's 2x2
up-convolution (padding 0), 3 the LinkNet / FCN form (padding 1, output_padding 1), 4 the pix2pix / DCGAN form (padding 1): each
doubles the plane exactly.  tools/configs.yml lists the type name, Reconstruction.ReconModel makes each a NewConvTranspose2d, and
resident.enable(..., concat=True, deconv=True) keeps them on the integers (fq_deconv2d_i8_resident).  With the defaults
(`up="bilinear"`, `up_kernel=2`) the model is what it was.

The reference ships no U-Net; this one is written from the architecture.  `base_width` is w (64 in the paper; tests build a narrow
network), `depth` the number of pools, `batch_norm=False` builds the network as merge_bn leaves it.  `input_size` must be a
multiple of 2^depth: every pool halves the plane and every skip must meet its upsampled partner at the same size.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat  # noqa: E402


def _level(cin, c, batch_norm=True):
    layers = []
    for a, b in ((cin, c), (c, c)):
        layers.append(nn.Conv2d(a, b, kernel_size=3, padding=1, bias=not batch_norm))
        if batch_norm:
            layers.append(nn.BatchNorm2d(b))
        layers.append(nn.ReLU(False))
    return nn.Sequential(*layers)


class UNet(nn.Module):

    # up_kernel -> (kernel, stride, padding, output_padding) of the up-convolution: each maps a plane of n to 2n
    UP_GEOMETRY = {2: (2, 2, 0, 0), 3: (3, 2, 1, 1), 4: (4, 2, 1, 0)}

    def __init__(self, num_classes=2, input_size=224, base_width=64, depth=4, batch_norm=True, in_channels=3, up="bilinear",
                 up_kernel=2):
        super(UNet, self).__init__()
        if up not in ("bilinear", "deconv"):
            raise ValueError("UNet: up must be 'bilinear' or 'deconv', got %r" % (up,))
        if isinstance(up_kernel, bool) or up_kernel not in self.UP_GEOMETRY:
            raise ValueError("UNet: up_kernel must be 2, 3 or 4, got %r" % (up_kernel,))
        if depth < 1 or base_width < 1:
            raise ValueError("UNet: depth and base_width must be positive, got %r and %r" % (depth, base_width))
        if input_size < (1 << depth) or input_size % (1 << depth):
            raise ValueError("UNet: input_size must be a multiple of 2^depth = %d (every skip meets its upsampled partner at the "
                             "same size), got %r" % (1 << depth, input_size))
        w = base_width
        self.depth = depth
        deconv = up == "deconv"
        widths = [w << i for i in range(depth)] + [w << (depth if deconv else depth - 1)]
        self.inc = _level(in_channels, widths[0], batch_norm)
        self.pools = nn.ModuleList(nn.MaxPool2d(2) for _ in range(depth))
        self.downs = nn.ModuleList(_level(widths[i], widths[i + 1], batch_norm) for i in range(depth))
        if deconv:
            k, s, p, op = self.UP_GEOMETRY[up_kernel]
            self.ups = nn.ModuleList(nn.ConvTranspose2d(2 * widths[depth - 1 - j], widths[depth - 1 - j], k, stride=s, padding=p,
                                                        output_padding=op) for j in range(depth))
        else:
            self.ups = nn.ModuleList(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) for _ in range(depth))
        self.Concats = nn.ModuleList(Concat() for _ in range(depth))
        # decoder step j joins skip depth-1-j (width widths[depth-1-j]) with the upsampled tensor of the same width
        outs = [widths[depth - 1 - j] if deconv else max(widths[depth - 1 - j] // 2, w) for j in range(depth)]
        self.decs = nn.ModuleList(_level(2 * widths[depth - 1 - j], outs[j], batch_norm) for j in range(depth))
        self.head = nn.Conv2d(w, num_classes, kernel_size=1)

    def forward(self, x):
        skips = [self.inc(x)]
        for pool, down in zip(self.pools, self.downs):
            skips.append(down(pool(skips[-1])))
        x = skips.pop()
        for up, cat, dec in zip(self.ups, self.Concats, self.decs):
            x = dec(cat(skips.pop(), up(x)))
        return self.head(x)
