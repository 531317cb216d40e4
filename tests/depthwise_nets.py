"""Small helpers shared by the depthwise tests (test infrastructure, no product code): integer-simulation models built from a
float model and a table of FIXED bits -- no calibration, so the CPU suite can build them too -- and one more separable toy net.

  fixed_info(model)   {layer name: info} for every Conv2d / Linear in registration order (= execution order in these nets): the
                      input bit of a layer is the output bit of the layer before it, as a calibration would give for a chain, so
                      that consecutive integer layers can hand integers to each other; weight bits from the weights' own range,
                      per tensor, per output channel (per_channel=True) or per channel for the grouped convolutions only
                      (per_channel="depthwise"), capped like MAX_SHIFT caps them (shift <= 12);
  rebuild(model, info)  the model with Conv2d / Linear / Eltwise swapped for NewConv2d / NewLinear / NewAdd (what
                      Reconstruction.ReconModel does, without the work directory).
"""
import copy
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from per_channel_chain import numpy_channel_bits


def fixed_info(model, per_channel=False, image_bit=5, seed=0, out_bits=(3, 4, 5), out_bit_of=None):
    rng = np.random.default_rng(seed)
    info = OrderedDict()
    ib = image_bit
    for name, m in model.named_modules():
        kind = type(m).__name__
        if kind not in ("Conv2d", "Linear"):
            continue
        ob = int(rng.choice(out_bits)) if out_bit_of is None else int(out_bit_of[name])
        wb0, tensor_bit = numpy_channel_bits(m.weight.detach().cpu().numpy())
        cap = 12 - ib + ob
        listed = per_channel is True or (per_channel == "depthwise" and kind == "Conv2d" and m.groups > 1)
        wb = [min(b, cap) for b in wb0] if listed else min(tensor_bit, cap)
        info[name] = {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob, "layer": m, "layer_type": kind}
        ib = ob
    return info


def rebuild(float_model, info):
    from common.quantity import NewConv2d, NewLinear, NewAdd
    model = copy.deepcopy(float_model)
    for name, mod in list(model.named_modules()):
        kind = type(mod).__name__
        if kind in ("Conv2d", "Linear"):
            q = {k: v for k, v in info[name].items() if k not in ("layer", "layer_type")}
            new = NewConv2d(mod, q) if kind == "Conv2d" else NewLinear(mod, q)
        elif kind == "Eltwise":
            new = NewAdd()
        else:
            continue
        parent = model
        for p in name.split(".")[:-1]:
            parent = getattr(parent, p)
        parent.add_module(name.split(".")[-1], new)
    return model.eval()


def shifts(info, name):
    """The right shifts of layer `name` as a list (one entry for per-tensor bits)."""
    q = info[name]
    wb = q["weight_bit"] if isinstance(q["weight_bit"], (list, tuple)) else [q["weight_bit"]]
    return [int(b) + q["input_bit"] - q["output_bit"] for b in wb]


class SeparableAddNet(nn.Module):
    """A depthwise layer whose output feeds an Eltwise DIRECTLY (no ReLU, no pointwise layer between), a 5x5 stride-2 depthwise
    layer, 19 channels (padded to 32 in the integer layout).  A module-level class, so the rebuilt model pickles."""

    def __init__(self):
        from common.quantity import Eltwise, View
        super(SeparableAddNet, self).__init__()
        self.stem = nn.Conv2d(3, 19, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.dwa = nn.Conv2d(19, 19, 3, padding=1, groups=19)
        self.Eltwise = Eltwise()
        self.r1 = nn.ReLU(False)
        self.dwb = nn.Conv2d(19, 19, 5, stride=2, padding=2, groups=19)
        self.r2 = nn.ReLU(False)
        self.pw = nn.Conv2d(19, 24, 1)
        self.r3 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(24, 5)

    def forward(self, x):
        x = self.r0(self.stem(x))
        x = self.r1(self.Eltwise(self.dwa(x), x))
        x = self.r3(self.pw(self.r2(self.dwb(x))))
        return self.fc(self.view(self.pool(x)))


def seeded(model, seed=3):
    """Deterministic weights with a spread that leaves the integer layers something to do (not all zeros, not all saturated)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=gen) * (1.5 / fan ** 0.5 if p.dim() > 1 else 0.2))
    return model


def measured_out_bits(model, x):
    """{layer name: output bit} from one float forward: 7 - ceil(log2(max |output|)) per Conv2d / Linear, the bit an abs-max
    calibration would give -- so that a big synthetic model keeps its activations inside the int8 range layer after layer
    (fixed_info(out_bit_of=...)), without running the calibration."""
    import math
    seen, hooks = {}, []
    for name, m in model.named_modules():
        if type(m).__name__ in ("Conv2d", "Linear"):
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, float(o.abs().max()))))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return {n: 7 - int(math.ceil(math.log2(v))) if v > 0 else 4 for n, v in seen.items()}
