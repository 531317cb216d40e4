"""Shared by the Concat / nearest-upsampling tests (test infrastructure, no product code): the kernel's case list, and small
integer-simulation nets built directly from NewConv2d info dicts -- no calibration, so the CPU suite (on the doubles of
tests/concat_doubles.py) and the GPU suite build the same nets.  Module-level classes, so a planned net pickles.

Bits: an image at bit 5, activations at bit 4 unless a test says otherwise; the two operands of a Concat get ONE output bit (what
the calibrator's merge group gives them) and the layer behind the Concat reads at that bit, so integers can be handed on.
"""
import math

import torch
from torch import nn

# (N, H, W, C0, C1, up0, up1); C1 == 0: one source (stand-alone nearest upsampling).  H, W are the OUTPUT plane.
TWO_SOURCE_CASES = [
    (2, 5, 7, 16, 16, 1, 1), (1, 4, 4, 64, 64, 1, 1),                      # aligned path
    (3, 7, 9, 20, 44, 1, 1),                                                # dword-aligned, not 16-byte-aligned
    (2, 3, 5, 3, 5, 1, 1), (1, 6, 6, 17, 30, 1, 1),                         # byte-unaligned; straddling chunks; Cpad_out 48 < 32 + 32
    (1, 2, 2, 13, 3, 1, 1),                                                 # sum == 16 exactly: no output padding
    (1, 1, 1, 1, 1, 1, 1),                                                  # single pixel, single channels
    (2, 8, 12, 24, 8, 1, 2), (1, 8, 8, 5, 7, 2, 1), (1, 8, 8, 16, 16, 4, 2),  # upsampled operands
    (2, 4, 6, 20, 44, 1, 2), (1, 4, 4, 17, 30, 2, 4),                       # ... whose dword and byte-shifted chunks read the upsampled one
]
ONE_SOURCE_CASES = [(2, hs * up, ws * up, C, 0, up, 1) for (C, up) in ((3, 2), (16, 2), (40, 4)) for (hs, ws) in ((2, 3), (5, 4))]
KERNEL_CASES = TWO_SOURCE_CASES + ONE_SOURCE_CASES


def case_arg(case):
    """The case as scripts/concat_geom_check.cpp reads it: N,H,W/C0,C1/up0,up1, one source as N,H,W/C0/up0."""
    N, H, W, c0, c1, u0, u1 = case
    return "%d,%d,%d/%d,%d/%d,%d" % case if c1 else "%d,%d,%d/%d/%d" % (N, H, W, c0, u0)


def conv(cin, cout, k, ib, ob, stride=1, padding=0, seed=0):
    """A NewConv2d over a seeded nn.Conv2d whose weights fill the int8 range at the weight bit chosen from their abs-max."""
    from common.quantity import NewConv2d
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + k + seed)
    c = nn.Conv2d(cin, cout, k, stride=stride, padding=padding)
    with torch.no_grad():
        c.weight.copy_(torch.randn(c.weight.shape, generator=gen) * (1.5 / (cin * k * k) ** 0.5))
        c.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
    wb = 7 - int(math.ceil(math.log2(float(c.weight.detach().abs().max()))))
    return NewConv2d(c, {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob})


class FireNet(nn.Module):
    """squeeze -> (expand 1x1 + ReLU, expand 3x3 + ReLU) -> Concat -> conv: 24 + 20 channels, so C0 is no multiple of 16."""

    def __init__(self, bits=(4, 4)):
        from common.quantity import Concat
        super(FireNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.squeeze, self.r1 = conv(16, 8, 1, 4, 4), nn.ReLU()
        self.e1, self.re1 = conv(8, 24, 1, 4, bits[0]), nn.ReLU()
        self.e3, self.re3 = conv(8, 20, 3, 4, bits[1], padding=1), nn.ReLU()
        self.cat = Concat()
        self.head, self.r2 = conv(44, 16, 1, bits[0], 4), nn.ReLU()
        self.branches = ("e1", "e3")

    def forward(self, x):
        s = self.r1(self.squeeze(self.r0(self.stem(x))))
        return self.r2(self.head(self.cat(self.re1(self.e1(s)), self.re3(self.e3(s)))))


class CatReluNet(nn.Module):
    """cases.tiny_concat_net's pattern: two convolutions -> Concat -> one ReLU behind it -> conv, then an Eltwise with a skip."""

    def __init__(self, bits=(4, 4), dim=1, dim_by_name=False):
        from common.quantity import Concat, NewAdd
        super(CatReluNet, self).__init__()
        self.stem, self.relu0 = conv(3, 8, 3, 5, 4, padding=1), nn.ReLU()
        self.branch_a = conv(8, 8, 3, 4, bits[0], padding=1)
        self.branch_b = conv(8, 8, 1, 4, bits[1])
        self.cat, self.relu1 = Concat(), nn.ReLU()
        self.mix = conv(16 if dim == 1 else 8, 8, 3, bits[0], 4, padding=1)
        self.skip = conv(8, 8, 1, 4, 4)
        self.add, self.relu2 = NewAdd(), nn.ReLU()
        self.dim, self.dim_by_name = dim, dim_by_name
        self.branches = ("branch_a", "branch_b")

    def forward(self, x):
        s = self.relu0(self.stem(x))
        a, b = self.branch_a(s), self.branch_b(s)
        c = self.cat(a, b, dim=self.dim) if self.dim_by_name else self.cat(a, b, self.dim)
        y = self.mix(self.relu1(c))
        if self.dim != 1:
            return y
        return self.relu2(self.add(y, self.skip(s)))


class FpnNet(nn.Module):
    """An FPN / YOLO style neck: coarse conv -> nearest upsampling -> Concat with a fine conv -> conv.  `shared`: the upsampled
    tensor is read by a second convolution as well, so it cannot be folded into the Concat.  `up`: the upsampling module."""

    def __init__(self, up=None, factor=2, shared=False, coarse_c=16):
        from common.quantity import Concat
        super(FpnNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.fine = conv(16, 24, 3, 4, 4, padding=1)
        self.down, self.r1 = conv(16, 32, 3, 4, 4, stride=factor, padding=1 if factor == 2 else 0), nn.ReLU()
        self.coarse = conv(32, coarse_c, 1, 4, 4)
        self.up = nn.UpsamplingNearest2d(scale_factor=factor) if up is None else up
        self.cat, self.r2 = Concat(), nn.ReLU()
        self.head = conv(coarse_c + 24, 16, 1, 4, 4)
        self.side = conv(coarse_c, 8, 1, 4, 4) if shared else None
        self.branches = ("fine", "coarse")

    def forward(self, x):
        s = self.r0(self.stem(x))
        u = self.up(self.coarse(self.r1(self.down(s))))
        y = self.head(self.r2(self.cat(u, self.fine(s))))
        return (y, self.side(u)) if self.side is not None else y


class CatAddNet(nn.Module):
    """A Concat output read by a resident NewAdd (and nothing else).  `add_operand`: instead, a NewAdd SUM is an operand of the
    Concat, which the plan leaves in fp32 form."""

    def __init__(self, add_operand=False):
        from common.quantity import Concat, NewAdd
        super(CatAddNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.a = conv(16, 16 if add_operand else 5, 1, 4, 4)
        self.b = conv(16, 16 if add_operand else 11, 3, 4, 4, padding=1)
        self.c = conv(16, 16, 1, 4, 4, seed=1)
        self.cat, self.add, self.r1 = Concat(), NewAdd(), nn.ReLU()
        self.head = conv(32 if add_operand else 16, 8, 1, 4, 4)
        self.add_operand = add_operand
        self.branches = ("a", "b")

    def forward(self, x):
        s = self.r0(self.stem(x))
        if self.add_operand:
            return self.head(self.r1(self.cat(self.add(self.a(s), self.b(s)), self.c(s))))
        return self.head(self.r1(self.add(self.cat(self.a(s), self.b(s)), self.c(s))))


def example(n=4, size=12, seed=1):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


DEFAULT_KEYS = {"resident_convs", "resident_adds", "resident_pools", "fused_relus", "fp32_outputs", "int_only_outputs",
                "fused_conv_adds", "fused_block_tails", "fused_projections"}


def squeezenet(size, classes=10, seed=0):
    """model/squeezenet/SqueezeNet_fabu.py with seeded weights whose spread keeps the activations alive through its 26 layers."""
    from model.squeezenet.SqueezeNet_fabu import SqueezeNet
    model = SqueezeNet(num_classes=classes, input_size=size)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=gen) * ((2.0 / fan) ** 0.5 if p.dim() > 1 else 0.05))
    return model.eval()


def squeezenet_info(model, out_bits, image_bit=5):
    """{layer name: info} for the SqueezeNet above WITHOUT a calibration: output bits from `out_bits` (one float forward's abs-max,
    depthwise_nets.measured_out_bits), the two expand layers of a Fire module share the smaller of their two bits (what the
    Concat merge group's pooled abs-max gives), and every layer reads at the bit its producer writes at."""
    from collections import OrderedDict

    from per_channel_chain import numpy_channel_bits
    info = OrderedDict()

    def put(name, m, ib, ob):
        _wb, tensor_bit = numpy_channel_bits(m.weight.detach().cpu().numpy())
        info[name] = {"weight_bit": min(tensor_bit, 12 - ib + ob), "bias_bit": ob, "input_bit": ib, "output_bit": ob, "layer": m,
                      "layer_type": "Conv2d"}
        return ob

    grid = put("conv1.0", model.conv1[0], image_bit, out_bits["conv1.0"])
    for n, m in model.features.named_children():
        if type(m).__name__ != "Fire":
            continue
        pre = "features.%s." % n
        s = put(pre + "squeeze", m.squeeze, grid, out_bits[pre + "squeeze"])
        grid = min(out_bits[pre + "expand1x1"], out_bits[pre + "expand3x3"])
        put(pre + "expand1x1", m.expand1x1, s, grid)
        put(pre + "expand3x3", m.expand3x3, s, grid)
    put("classifier.0", model.classifier[0], grid, out_bits["classifier.0"])
    return info
