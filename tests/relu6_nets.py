"""The small MobileNetV2 of golden G18 and of the ReLU6 tests (test infrastructure, no product code).

  g18_net()           model/mobilenetv2/MobileNetV2_fabu.py at width 0.5 on 32 x 32 images without BatchNorm (the network as
                      merge_bn leaves it): a 3 -> 16 stem, a t = 1 block (16 -> 24), a stride-2 block (24 -> 24, hidden 48), a
                      block with a shortcut (24 -> 24), a second stride-2 block (24 -> 32), a 1x1 to 64, a 4 x 4 average pool, a
                      Linear to 10 classes.  Every width lies in [16, 64].  The model file is loaded by PATH, so that it takes
                      Eltwise / View from whichever `common` package is imported (the golden script imports the reference's).
  integer_weights(m)  FIXED integer-valued weights and biases, drawn per tensor from a generator keyed by its state_dict name
                      (as cases.seed_model does).  The ranges are chosen so that the calibrated output bits put the clip of a
                      ReLU6 at work: the stem, a depthwise and a 1x1 expansion get output_bit <= 4 with values at the bound, and
                      the t = 1 block's depthwise layer, a centre tap of -1 with a bias of 3, stays below 4: output_bit >= 5, where
                      the clip is a plain ReLU.  tests/golden/make_golden_relu6.py asserts exactly that on the reference's run.
  integer_batches / integer_input   integer-valued images in [-8, 8].
On integer-valued data every fp32 partial sum of the float forward is an integer far below 2^24, so every engine computes the
same tensors bit for bit and the tables can be compared byte for byte.
"""
import importlib.util
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_FILE = os.path.join(os.path.dirname(HERE), "pytorch-quantity_amd", "quantity", "model", "mobilenetv2", "MobileNetV2_fabu.py")

G18_SHAPE = (4, 3, 32, 32)
G18_SEED, G18_CALIB_SEED, G18_INPUT_SEED = 18, 1800, 1818
G18_STAGES = ((1, 48, 1, 1), (2, 48, 2, 2), (2, 64, 1, 2))
NUM_CLASSES = 10
# the layers whose ReLU6 the data puts to work (output_bit <= 4, outputs at the bound), and the one where it is a plain ReLU
CLIPPED = ("conv1.0", "blocks.1.expand.0", "blocks.1.dw.0")
UNCLIPPED = ("blocks.0.dw.0",)


def _model_module():
    """The model file as a module of its own name (in sys.modules: ReconModel pickles the model), loaded anew whenever the
    `common` package it took Eltwise / View from is no longer the imported one."""
    name = "_fq_mobilenetv2_fabu"
    mod = sys.modules.get(name)
    if mod is not None and sys.modules.get(mod.Eltwise.__module__.split(".")[0]) is not None \
            and getattr(sys.modules.get(mod.Eltwise.__module__), "Eltwise", None) is mod.Eltwise:
        return mod
    spec = importlib.util.spec_from_file_location(name, MODEL_FILE)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def g18_net():
    return _model_module().MobileNetV2(num_classes=NUM_CLASSES, width_mult=0.5, input_size=G18_SHAPE[2], stages=G18_STAGES,
                                       last_width=64, batch_norm=False)


def integer_weights(model, base_seed=G18_SEED):
    import torch
    sd = model.state_dict()
    with torch.no_grad():
        for key in sorted(sd.keys()):
            t = sd[key]
            g = np.random.default_rng(base_seed * 1000003 + zlib.crc32(key.encode()))
            shape = tuple(t.shape)
            if key == "blocks.0.dw.0.weight":                 # the centre tap alone: the layer hands on its input, negated ...
                v = np.zeros(shape, dtype=np.float32)         # (negated: a pure shift of the input would have the input's
                v[:, :, 1, 1] = -1                            #  fingerprint in the reference's value-based graph discovery)
            elif key == "blocks.0.dw.0.bias":                 # ... and raised by 3: [0, 6] -> [-3, 3], below 4
                v = np.full(shape, 3, dtype=np.float32)
            elif t.dim() == 1:                                # a bias
                v = g.integers(-2, 3, shape).astype(np.float32)
            elif t.dim() == 4 and shape[1] == 1:              # depthwise 3x3: sparse, mostly positive
                v = (g.integers(-1, 3, shape) * (g.random(shape) < 0.6)).astype(np.float32)
            elif ".project." in key:                          # linear projection: very sparse, entries in [-1, 1]
                v = (g.integers(-1, 2, shape) * (g.random(shape) < 3.0 / int(np.prod(shape[1:])))).astype(np.float32)
            else:                                             # dense: sparse, entries in [-2, 2]
                fan_in = int(np.prod(shape[1:]))
                keep = min(1.0, 6.0 / fan_in)
                v = (g.integers(-2, 3, shape) * (g.random(shape) < keep)).astype(np.float32)
            t.copy_(torch.from_numpy(v))
    return model


def integer_batches(n_batches, shape=G18_SHAPE, seed=G18_CALIB_SEED):
    """(images, labels) pairs as cases.calib_batches gives them, the images integer valued in [-8, 8]."""
    import torch
    return [(torch.from_numpy(np.random.default_rng(seed + i).integers(-8, 9, tuple(shape)).astype(np.float32)),
             torch.zeros(shape[0], dtype=torch.long)) for i in range(n_batches)]


def integer_input(shape=G18_SHAPE, seed=G18_INPUT_SEED):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(-8, 9, tuple(shape)).astype(np.float32))


def bound_counts(model, x):
    """{conv name: (values of its output equal to 6 after the ReLU6 -- at or above the bound before it --, values strictly
    between 0 and 6)} for every convolution directly followed by an nn.ReLU6, on the float model."""
    import torch
    names = dict((m, n) for n, m in model.named_modules())
    last, out, hooks = [None], {}, []

    def conv_hook(m, _args, y):
        last[0] = (m, y)

    def relu_hook(_m, args, _y):
        if last[0] is not None and last[0][1] is args[0]:
            y = last[0][1]
            out[names[last[0][0]]] = (int((y >= 6).sum()), int(((y > 0) & (y < 6)).sum()))

    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            hooks.append(m.register_forward_hook(conv_hook))
        elif isinstance(m, torch.nn.ReLU6):
            hooks.append(m.register_forward_hook(relu_hook))
    try:
        with torch.no_grad():
            model(x)
    finally:
        for h in hooks:
            h.remove()
    return out
