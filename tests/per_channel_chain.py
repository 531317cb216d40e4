"""Expected values for per-channel weight bits (test infrastructure, no product code).

  pc_epilogue      the oracle's recon_epilogue (RightShift -> BiasAdd -> Sp -> DeQuantity) applied one output-channel slice
                   at a time with that channel's shift;
  cpu_chain        the reference's ReconModel structure as torch-CPU modules in fp32 with the shift taken per output
                   channel: Quantity -> contraction -> per-channel tail per Conv2d / Linear, NewAdd's saturation per Eltwise,
                   every other module (ReLU, pooling, View) the model's own on the CPU.  The contraction runs in float64 on
                   the integer-valued operands, which is exact (|partial sums| < 2^53), and is cast back to fp32;
  numpy_channel_bits  the per-channel bits of weight_quantize_per_channel recomputed from the float weights with NumPy.
"""
import copy
import math

import numpy as np
import torch
import torch.nn as nn

from oracle import fq_oracle as orc


def pc_epilogue(acc, qbias, rs, ob):
    """acc fp32 [N, K, ...] (ndarray), qbias fp32[K], rs: K shifts -> fp32 ndarray."""
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    out = np.empty_like(acc)
    for c in range(acc.shape[1]):
        out[:, c:c + 1] = orc.recon_epilogue(np.ascontiguousarray(acc[:, c:c + 1]), np.asarray(qbias, np.float32)[c:c + 1],
                                             int(rs[c]), int(ob))
    return out


def quantize_rows(w, bits):
    """clip(round_half_even(w[c] * 2^bits[c]), -128, 127), fp32, the reference's torch expression per output channel."""
    out = torch.empty_like(w)
    for c, b in enumerate(bits):
        out[c] = torch.round(torch.mul(w[c], pow(2, int(b)))).clamp(-128, 127)
    return out


def _bits_list(bit, k):
    return [int(b) for b in bit] if isinstance(bit, (list, tuple)) else [int(bit)] * k


class ChainLayer(nn.Module):
    """One Conv2d / Linear of the reference ReconModel with per-channel shifts, on the CPU."""

    def __init__(self, layer, info):
        super(ChainLayer, self).__init__()
        k = layer.out_channels if isinstance(layer, nn.Conv2d) else layer.out_features
        self.wb = _bits_list(info["weight_bit"], k)
        self.ib, self.ob = int(info["input_bit"]), int(info["output_bit"])
        self.rs = [b + self.ib - self.ob for b in self.wb]
        lay = copy.deepcopy(layer).cpu().float()
        wq = quantize_rows(lay.weight.data, self.wb)
        b = lay.bias.data if lay.bias is not None else torch.zeros(k)
        self.qb = torch.round(torch.mul(b, pow(2, int(info["bias_bit"])))).clamp(-128, 127)
        lay.weight = nn.Parameter(wq.double())
        lay.bias = None
        self.layer = lay

    def forward(self, x):
        with torch.no_grad():
            q = torch.round(torch.mul(x.detach().float(), pow(2, self.ib))).clamp(-128, 127)
            acc = self.layer(q.double()).float()
        return torch.from_numpy(pc_epilogue(acc.numpy(), self.qb.detach().numpy(), self.rs, self.ob))


class ChainAdd(nn.Module):
    def forward(self, x, y):
        return torch.clamp(x + y, -128.0, 127.0)


def cpu_chain(float_model, info):
    """A CPU copy of the merged float model with every Conv2d / Linear / Eltwise replaced as described above."""
    model = copy.deepcopy(float_model).cpu().float().eval()
    for name, module in list(model.named_modules()):
        kind = type(module).__name__
        if kind in ("Conv2d", "Linear"):
            new = ChainLayer(module, info[name])
        elif kind == "Eltwise":
            new = ChainAdd()
        else:
            continue
        parent = model
        parts = name.split(".")
        for p in parts[:-1]:
            parent = getattr(parent, p)
        parent.add_module(parts[-1], new)
    return model


def numpy_channel_bits(w):
    """(wb0 per output channel, the tensor's bit) of a float weight ndarray [K, ...], as weight_quantize_per_channel defines them."""
    w = np.asarray(w, dtype=np.float32)
    m = np.abs(w.reshape(w.shape[0], -1)).max(axis=1)
    tensor_bit = int(8 - 1 - math.ceil(math.log(float(m.max()), 2)))
    return [int(8 - 1 - math.ceil(math.log(float(v), 2))) if v > 0 else tensor_bit for v in m], tensor_bit


def dilate_dense(w, dilation):
    """weight_quantize's dilation_to_zero_padding for a dilation-2 kernel, on a host tensor."""
    k = w.shape[2]
    dense = torch.zeros(w.shape[0], w.shape[1], 2 * k - 1, 2 * k - 1)
    dense[..., ::2, ::2] = w
    return dense

