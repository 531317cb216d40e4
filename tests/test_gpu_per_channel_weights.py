"""Per-channel weight bits on the MI355X: the _pcs entry points of every integer convolution kernel against the CPU oracle,
the per-channel epilogue, NewConv2d / NewLinear / ReconModel / ReconTest with list bits against the CPU chain
(tests/per_channel_chain.py), the resident planner, and the accuracy gain on a layer whose folded channel scales spread.

Kernel-level expected values: the oracle's integer convolution with recon_epilogue applied one channel slice at a time.  For
the shapes that only a large launch selects (halo8, dma2, 128-row tiles) the oracle would take minutes on the CPU; there the
expected value is the PER-TENSOR entry point run once per distinct shift, channel by channel.  That entry point, and the _pcs
one with it, is compared at these very shapes with an exact float64 convolution by test_gpu_conv_i8_large.py (whose case-list
test checks that every such row of SHAPES is in its table); test_gpu_conv_i8.py covers the small launches.  pytest -m gpu"""
import copy
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
from per_channel_chain import ChainLayer, cpu_chain, numpy_channel_bits, pc_epilogue, quantize_rows
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu


def _nat():
    from common.quantity import _native
    return _native


def _shift(rs, dev="cuda"):
    nat = _nat()
    return nat.ShiftVec(torch.tensor(rs, dtype=torch.int32, device=dev), min(rs), max(rs))


def _operands(rng, N, H, W, C, K, R, S, bias_scale=200.0, big_bias=True):
    x = rng.integers(-128, 128, (N, C, H, W)).astype(np.int32)
    w = rng.integers(-128, 128, (K, C, R, S)).astype(np.int32)
    qb = np.rint(rng.standard_normal(K) * bias_scale).astype(np.float32)
    if big_bias:
        qb[:3] = [3.0e6, -2.5e6, 127.0][:min(3, K)]
    return x, w, qb


def _dev(nat, x, w, qb):
    xq = nat.quantize_i8_nhwc(torch.from_numpy(x.astype(np.float32)).cuda(), 0)
    wq = nat.pack_weight_krsc(torch.from_numpy(w.astype(np.float32)).cuda())
    return xq, wq, torch.from_numpy(qb).cuda()


def _spread(rng, K, lo=1, hi=12):
    rs = rng.integers(lo, hi + 1, K).tolist()
    rs[0], rs[-1] = lo, hi
    return rs


def _composed(fn, rs):
    """The per-tensor entry point `fn(rs_value)` -> tuple of outputs, composed channel by channel: channel k from the call with
    rs[k].  Outputs are fp32 NCHW (channel axis 1) or integer NHWC (channel axis -1), or None."""
    parts = {v: fn(v) for v in sorted(set(rs))}
    first = parts[rs[0]]
    out = []
    for i, t in enumerate(first):
        if t is None:
            out.append(None)
            continue
        axis = 1 if t.dtype == torch.float32 else t.dim() - 1
        res = t.clone()
        for k, v in enumerate(rs):
            res.select(axis, k).copy_(parts[v][i].select(axis, k))
        out.append(res)
    return out


# (name, N, H, W, C, K, R, S, stride, pad, expected variant, oracle-checked)
SHAPES = [
    ("c64_halo", 2, 12, 12, 64, 64, 3, 3, 1, 1, "c64_halo/64", True),
    ("halo", 2, 10, 10, 128, 64, 3, 3, 1, 1, "halo/64", True),
    ("halo8", 64, 32, 32, 128, 64, 3, 3, 1, 1, "halo8/64", False),
    ("dma3", 2, 10, 10, 128, 64, 3, 3, 2, 1, "dma3/64", True),
    ("dma2", 40, 64, 64, 128, 64, 3, 3, 2, 1, "dma2/64", False),
    ("tile_c128", 2, 8, 8, 128, 64, 1, 1, 1, 0, "tile_c128/64", True),
    ("tile_c64", 2, 9, 7, 64, 96, 1, 1, 1, 0, "tile_c64/64", True),
    ("tile_general", 2, 9, 11, 48, 40, 3, 3, 1, 1, "tile_general/64", True),
    ("tile_general_128", 8, 64, 64, 48, 160, 1, 1, 1, 0, "tile_general/128", False),
    ("tile_c128_128", 32, 32, 32, 128, 256, 1, 1, 1, 0, "tile_c128/128", False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("tail", ["int", "fp32"])
def test_conv_pcs_every_variant(oracle, shape, tail):
    nat = _nat()
    name, N, H, W, C, K, R, S, st, pd, variant, small = shape
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + (tail == "fp32"))
    x, w, qb = _operands(rng, N, H, W, C, K, R, S)
    xq, wq, qbd = _dev(nat, x, w, qb)
    rs = _spread(rng, K) if tail == "int" else _spread(rng, K, -2, 19)
    ob = 3
    geom = ((st, st), (pd, pd), (1, 1))
    rsv = _shift(rs)
    nat.conv_variant_log = {}
    try:
        y = nat.conv2d_i8(xq, wq, qbd, *geom, rsv, ob)
        log = dict(nat.conv_variant_log)
    finally:
        nat.conv_variant_log = None
    assert log == {variant: 1}, log
    if small:
        acc = oracle.conv2d_int(x, w, stride=(st, st), pad=(pd, pd)).astype(np.float32)
        np.testing.assert_array_equal(y.cpu().numpy(), pc_epilogue(acc, qb, rs, ob))
    exp = _composed(lambda v: (nat.conv2d_i8(xq, wq, qbd, *geom, v, ob),), rs)[0]
    assert torch.equal(y, exp)
    # resident outputs (fp32 + int8 NHWC, ReLU on and off) and the fused residual add, where the variant takes them
    for relu in (False, True):
        got = nat.conv2d_i8_resident(xq, wq, qbd, *geom, rsv, ob, True, True, relu)
        exp = _composed(lambda v: nat.conv2d_i8_resident(xq, wq, qbd, *geom, v, ob, True, True, relu), rs)
        assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1])
        if small and relu:
            ref = np.maximum(pc_epilogue(acc, qb, rs, ob), 0)
            np.testing.assert_array_equal(got[0].cpu().numpy(), ref)
            np.testing.assert_array_equal(np.moveaxis(got[1].cpu().numpy()[..., :K], -1, 1).astype(np.float32), ref * 2.0 ** ob)
    res = torch.from_numpy(rng.integers(-128, 128, tuple(got[1].shape)).astype(np.int8)).cuda()
    res[..., K:] = 0
    for g_res in (2, 5):
        got = nat.conv2d_i8_add_resident(xq, wq, qbd, *geom, rsv, ob, res, g_res, True, max(0, ob, g_res), True, 4, False)
        exp = _composed(lambda v: nat.conv2d_i8_add_resident(xq, wq, qbd, *geom, v, ob, res, g_res, True, max(0, ob, g_res), True, 4,
                                                             False), rs)
        assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1])


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_conv_pcs_constant_vector_is_the_per_tensor_entry_point(shape):
    nat = _nat()
    name, N, H, W, C, K, R, S, st, pd, variant, _small = shape
    rng = np.random.default_rng(7)
    x, w, qb = _operands(rng, N, H, W, C, K, R, S)
    xq, wq, qbd = _dev(nat, x, w, qb)
    geom = ((st, st), (pd, pd), (1, 1))
    for rs in (1, 7, 16, 0, 20):
        rsv = _shift([rs] * K)
        assert torch.equal(nat.conv2d_i8(xq, wq, qbd, *geom, rsv, 2), nat.conv2d_i8(xq, wq, qbd, *geom, rs, 2))
        a = nat.conv2d_i8_resident(xq, wq, qbd, *geom, rsv, 2, True, True, True)
        b = nat.conv2d_i8_resident(xq, wq, qbd, *geom, rs, 2, True, True, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = nat.conv2d_i8_resident(xq, wq, qbd, *geom, rsv, 2, False, True, False)
        b = nat.conv2d_i8_resident(xq, wq, qbd, *geom, rs, 2, False, True, False)
        assert torch.equal(a[1], b[1])


@pytest.mark.parametrize("tail", ["int", "fp32"])
def test_linear_wave_pcs(oracle, tail):
    nat = _nat()
    rng = np.random.default_rng(3)
    N, C, K = 5, 200, 37
    x = rng.integers(-128, 128, (N, C)).astype(np.int32)
    w = rng.integers(-128, 128, (K, C)).astype(np.int32)
    qb = np.rint(rng.standard_normal(K) * 300).astype(np.float32)
    qb[0] = 5.0e6
    xq = nat.quantize_i8_nhwc(torch.from_numpy(x.astype(np.float32)).cuda(), 0)
    wq = nat.pack_weight_krsc(torch.from_numpy(w.astype(np.float32)).cuda())
    rs = _spread(rng, K) if tail == "int" else _spread(rng, K, 0, 18)
    nat.conv_variant_log = {}
    try:
        y = nat.conv2d_i8(xq, wq, torch.from_numpy(qb).cuda(), (1, 1), (0, 0), (1, 1), _shift(rs), 1)
        log = dict(nat.conv_variant_log)
    finally:
        nat.conv_variant_log = None
    assert log == {"linear_wave/32": 1}, log
    acc = (x.astype(np.int64) @ w.T.astype(np.int64)).astype(np.float32)
    np.testing.assert_array_equal(y.cpu().numpy(), pc_epilogue(acc, qb, rs, 1))
    same = nat.conv2d_i8(xq, wq, torch.from_numpy(qb).cuda(), (1, 1), (0, 0), (1, 1), _shift([6] * K), 1)
    assert torch.equal(same, nat.conv2d_i8(xq, wq, torch.from_numpy(qb).cuda(), (1, 1), (0, 0), (1, 1), 6, 1))


@pytest.mark.parametrize("shape", [(3, 20, 7, 9), (2, 24, 8, 8), (4, 10)])
def test_recon_epilogue_pcs(oracle, shape):
    nat = _nat()
    rng = np.random.default_rng(len(shape))
    acc = np.rint(rng.standard_normal(shape) * 3.0e4).astype(np.float32)
    acc.flat[:4] = [2.0 ** 30, -2.0 ** 30, 1.5, -2.5]
    K = shape[1]
    qb = np.rint(rng.standard_normal(K) * 100).astype(np.float32)
    rs = rng.integers(-3, 20, K).tolist()
    y = nat.recon_epilogue(torch.from_numpy(acc).cuda(), torch.from_numpy(qb).cuda(), _shift(rs), 2)
    np.testing.assert_array_equal(y.cpu().numpy(), pc_epilogue(acc, qb, rs, 2))
    const = nat.recon_epilogue(torch.from_numpy(acc).cuda(), torch.from_numpy(qb).cuda(), _shift([5] * K), 2)
    assert torch.equal(const, nat.recon_epilogue(torch.from_numpy(acc).cuda(), torch.from_numpy(qb).cuda(), 5, 2))


def test_pcs_bounds_are_checked():
    nat = _nat()
    xq = torch.zeros(1, 4, 4, 16, dtype=torch.int8, device="cuda")
    wq = torch.zeros(8, 1, 1, 16, dtype=torch.int8, device="cuda")
    qb = torch.zeros(8, device="cuda")
    with pytest.raises(nat.FqError):
        nat.conv2d_i8(xq, wq, qb, (1, 1), (0, 0), (1, 1), _shift([1] * 7), 0)              # one shift short
    with pytest.raises(nat.FqError):
        nat.conv2d_i8(xq, wq, qb, (1, 1), (0, 0), (1, 1), nat.ShiftVec(torch.zeros(8, dtype=torch.int32, device="cuda"), 0, 121), 0)
    # the stem and block-tail kernels have the integer tail only: a shift outside [1, 16] keeps the layer on the general kernels
    assert nat.stem_supported(3, 16, 3, 3, (1, 1), (1, 1), _shift([2] * 16))
    assert not nat.stem_supported(3, 16, 3, 3, (1, 1), (1, 1), _shift([2] * 15 + [17]))
    assert nat.block_tail_supported(64, 128, 0, _shift([2] * 128), 0, 3, 3, 1, 2)
    assert not nat.block_tail_supported(64, 128, 0, _shift([0] + [2] * 127), 0, 3, 3, 1, 2)


# ---- modules -------------------------------------------------------------------------------------------------------------

def oracle_rightshift(x, rs):
    from oracle import fq_oracle as orc
    return orc.recon_epilogue(x.reshape(x.shape[0], 1, -1), np.zeros(1, np.float32), int(rs), 0).reshape(x.shape)


def _layers():
    g = torch.Generator().manual_seed(21)
    out = []
    for name, mod in [("conv", nn.Conv2d(24, 40, 3, padding=1)), ("grouped", nn.Conv2d(32, 48, 3, padding=1, groups=4)),
                      ("depthwise", nn.Conv2d(32, 32, 3, stride=2, padding=1, groups=32)),
                      ("circular", nn.Conv2d(16, 24, 3, padding=1, padding_mode="circular")),
                      ("linear", nn.Linear(96, 33))]:
        with torch.no_grad():
            mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.2)
            k = mod.weight.shape[0]
            mod.weight.mul_(torch.pow(2.0, -torch.arange(k, dtype=torch.float32) % 9).view(-1, *([1] * (mod.weight.dim() - 1))))
            mod.bias.copy_(torch.randn(k, generator=g) * 0.3)
        out.append((name, mod))
    return out


@pytest.mark.parametrize("idx", range(5), ids=["conv", "grouped", "depthwise", "circular", "linear"])
def test_modules_with_list_bits_equal_the_chain(idx):
    from common.quantity import NewConv2d, NewLinear
    name, mod = _layers()[idx]
    wb0, _tb = numpy_channel_bits(mod.weight.detach().numpy())
    info = {"weight_bit": [min(b, 13) for b in wb0], "bias_bit": 4, "input_bit": 3, "output_bit": 4}
    assert len(set(info["weight_bit"])) > 4
    cls = NewLinear if name == "linear" else NewConv2d
    shape = (6, 96) if name == "linear" else (3, mod.in_channels, 10, 9)
    x = torch.from_numpy(np.random.default_rng(idx).standard_normal(shape).astype(np.float32) * 4)
    ref = ChainLayer(mod, info)(x)
    layer = cls(copy.deepcopy(mod).cuda(), info)
    with torch.no_grad():
        y = layer(x.cuda())
    np.testing.assert_array_equal(y.cpu().numpy(), ref.numpy())
    # the RightShift submodule of the reference structure shifts channel by channel
    acc = torch.from_numpy(np.random.default_rng(5).integers(-40000, 40000, (2, len(info["weight_bit"]), 3)).astype(np.float32)).cuda()
    rsm = layer.RightShift(acc).cpu().numpy()
    for c, r in enumerate(layer.rs_bit):
        assert np.array_equal(rsm[:, c], oracle_rightshift(acc[:, c].cpu().numpy(), r))
    # every bit the same: the per-tensor layer, bit for bit
    k = len(info["weight_bit"])
    a = cls(copy.deepcopy(mod).cuda(), dict(info, weight_bit=[9] * k))
    b = cls(copy.deepcopy(mod).cuda(), dict(info, weight_bit=9))
    with torch.no_grad():
        assert torch.equal(a(x.cuda()), b(x.cuda()))


# ---- models --------------------------------------------------------------------------------------------------------------

def _fake_quant_chain(float_model, info):
    """CPU counterpart of ReconTest with per-channel weight bits: weights fake-quantised per channel, bias at bias_bit, every
    output quantised -> dequantised at output_bit, NewAdd's saturation per Eltwise."""
    from per_channel_chain import ChainAdd
    model = copy.deepcopy(float_model).cpu().float().eval()

    class FQ(nn.Module):
        def __init__(self, layer, q):
            super(FQ, self).__init__()
            k = layer.weight.shape[0]
            wb = q["weight_bit"] if isinstance(q["weight_bit"], list) else [q["weight_bit"]] * k
            w = quantize_rows(layer.weight.data, wb) / torch.pow(2.0, torch.tensor(wb, dtype=torch.float32)).view(
                -1, *([1] * (layer.weight.dim() - 1)))
            s = pow(2, q["bias_bit"])
            b = torch.round(torch.mul(layer.bias.data, s)).clamp(-128, 127) / s
            layer.weight, layer.bias = nn.Parameter(w), nn.Parameter(b)
            self.layer, self.ob = layer, q["output_bit"]

        def forward(self, x):
            s = pow(2, self.ob)
            return torch.round(torch.mul(self.layer(x), s)).clamp(-128, 127) / s

    for name, module in list(model.named_modules()):
        kind = type(module).__name__
        new = FQ(module, info[name]) if kind in ("Conv2d", "Linear") else (ChainAdd() if kind == "Eltwise" else None)
        if new is None:
            continue
        parent = model
        for p in name.split(".")[:-1]:
            parent = getattr(parent, p)
        parent.add_module(name.split(".")[-1], new)
    return model


def _model(kind):
    from common.quantity import merge_bn
    if kind == "r18":
        from model.resnet.ResNet_18_fabu import ResNet18
        return merge_bn(cases.seed_model(ResNet18()).eval()), (4, 3, 32, 32)
    return merge_bn(cases.seed_model(cases.tiny_separable_net()).eval()), (4, 3, 16, 16)


@pytest.mark.parametrize("kind", ["r18", "separable"])
def test_per_channel_model_end_to_end(kind, monkeypatch):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    float_model, shape = _model(kind)
    if kind == "separable":
        monkeypatch.setattr(torch, "save", lambda *a, **k: None)       # the fixture net is a local class: not picklable
    with product_workdir(input_shape=",".join(str(v) for v in (1,) + shape[1:]), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(copy.deepcopy(float_model).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        capped = q.weight_quantize_per_channel()
        feat = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in open(os.path.join(wd, "feat.table")) if ln.strip()}
        # bits and JSON against NumPy, from the float weights
        table = open(os.path.join(wd, "weight_channel.table")).read().splitlines()
        spread = 0
        for name, p in float_model.named_parameters():
            layer = name.rsplit(".", 1)[0]
            row = [ln for ln in table if ln.split()[0] == name]
            assert len(row) == 1, name
            if name.endswith(".bias"):
                assert row[0].split()[1:] == [str(feat[layer][0])]
                continue
            wb0, _tb = numpy_channel_bits(p.detach().numpy())
            wb = [min(b, 12 - feat[layer][1] + feat[layer][0]) for b in wb0]
            assert [int(v) for v in row[0].split()[1:]] == wb == capped[layer]
            spread = max(spread, len(set(wb)))
            import json
            got = np.array(json.load(open(os.path.join(wd, "weight_channel", name + ".json"))))
            w = p.detach().numpy()
            exp = np.stack([np.clip(np.rint(w[c] * np.float32(2.0 ** b)), -128, 127) for c, b in enumerate(wb0)])
            np.testing.assert_array_equal(got, exp)
        assert spread > 1
        rec = Reconstruction(copy.deepcopy(float_model))
        info = rec.get_quantity_information_per_channel()
        net = rec.ReconModel(info, os.path.join(wd, "recon_pc.pth")).cuda()
        chain = cpu_chain(float_model, info)
        x = cases.fixed_input(shape)
        with torch.no_grad():
            logits = net(x.cuda())
            ref = chain(x)
        np.testing.assert_array_equal(logits.cpu().numpy(), ref.numpy())
        if kind == "r18":                                              # save / load round trip
            again = torch.load(os.path.join(wd, "recon_pc.pth"), weights_only=False).cuda()
            with torch.no_grad():
                assert torch.equal(again(x.cuda()), logits)
            assert sorted(again.state_dict().keys()) == sorted(net.state_dict().keys())
            assert all(not k.endswith("rs_vec") for k in net.state_dict())
        plan = resident.enable(net, x.cuda(), verify=True)
        with torch.no_grad():
            assert torch.equal(net(x.cuda()), logits)
        assert plan["resident_convs"] > 0
        # ReconTest: the tolerance of test_gpu_e2e.py (one quantisation step of the last layer)
        rt = Reconstruction(copy.deepcopy(float_model)).ReconTest(info, os.path.join(wd, "recontest_pc.pth")).cuda()
        with torch.no_grad():
            fl = rt(x.cuda()).cpu()
            fref = _fake_quant_chain(float_model, info)(x)
        last = [n for n, m in float_model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))][-1]
        assert float((fl - fref).abs().max()) <= 2.0 ** -info[last]["output_bit"] + 1e-6


def _r50_info(model, seed=0):
    """Synthetic per-channel bits for ResNet-50 (the resident planner's equality needs no calibration): per-channel bits from
    the folded weights, input / output bits of a plausible calibration."""
    from collections import OrderedDict
    rng = np.random.default_rng(seed)
    info = OrderedDict()
    for name, m in model.named_modules():
        kind = type(m).__name__
        if kind in ("Conv2d", "Linear"):
            wb0, _ = numpy_channel_bits(m.weight.detach().numpy())
            ib, ob = int(rng.integers(3, 6)), int(rng.integers(2, 5))
            info[name] = {"weight_bit": [min(b, 12 - ib + ob) for b in wb0], "bias_bit": ob, "input_bit": ib, "output_bit": ob,
                          "layer": m, "layer_type": kind}
    return info


def test_r50_per_channel_resident_and_chain():
    """ResNet-50 at 224 x 224, 256 images (the benchmark's dispatch size): resident per-channel logits equal the plain
    per-channel logits; every kernel launch of the per-tensor model (block tails and stem included) is the same variant for the
    per-channel one; a 2-image slice equals the CPU chain."""
    from common.quantity import NewConv2d, NewLinear, resident
    from common.quantity import merge_bn
    from model.resnet.ResNet_fabu import ResNet50
    nat = _nat()
    float_model = merge_bn(cases.seed_model(ResNet50(input_size=224)).eval())
    info = _r50_info(float_model)

    def build(per_channel):
        m = copy.deepcopy(float_model)
        for name, mod in list(m.named_modules()):
            if name in info:
                q = dict(info[name])
                if not per_channel:
                    q["weight_bit"] = min(q["weight_bit"])
                new = NewConv2d(mod, q) if isinstance(mod, nn.Conv2d) else NewLinear(mod, q)
                parent = m
                for p in name.split(".")[:-1]:
                    parent = getattr(parent, p)
                parent.add_module(name.split(".")[-1], new)
        return m.cuda()

    x = cases.fixed_input((256, 3, 224, 224)).cuda()
    pc = build(True)
    with torch.no_grad():
        plain = pc(x)
    logs = {}
    for key, net in (("pc", pc), ("pt", build(False))):
        resident.enable(net, x, verify=True)
        nat.conv_variant_log = {}
        try:
            with torch.no_grad():
                out = net(x)
            logs[key] = dict(nat.conv_variant_log)
        finally:
            nat.conv_variant_log = None
        if key == "pc":
            assert torch.equal(out, plain)
    assert logs["pc"] == logs["pt"], (logs["pc"], logs["pt"])            # no layer falls off its kernel
    with torch.no_grad():
        ref = cpu_chain(float_model, info)(x[:2].cpu())
    np.testing.assert_array_equal(plain[:2].cpu().numpy(), ref.numpy())


def test_per_channel_bits_halve_the_error_of_small_channels():
    """A 3x3 conv, 32 -> 36 channels, whose folded channel scales span 2^0 ... 2^-8 (BatchNorm running variances set before
    merge_bn, seed 0); every output channel carries one large tap (32 sigma), which sets the per-tensor bit.  The channels scaled
    by <= 2^-4 are compared with the float output.  Input / output bits from the data, weight bits capped at MAX_SHIFT = 12.
    Ratio per-channel / per-tensor mean squared error, measured with the CPU chain (per_channel_chain.ChainLayer, same seed
    and input): 0.217 (0.217 / 0.221 with seeds 1 / 2).  Without the large tap the shared output bit's rounding dominates
    both errors (0.69 - 0.82).  The test asks for <= 0.5."""
    from common.quantity import NewConv2d, merge_bn
    ratio = _accuracy_ratio(lambda mod, info, x: NewConv2d(copy.deepcopy(mod).cuda(), info)(x.cuda()).cpu(), merge_bn)
    assert ratio <= 0.5, ratio


def _accuracy_ratio(run, merge_bn, seed=0):
    torch.manual_seed(seed)
    seq = nn.Sequential(nn.Conv2d(32, 36, 3, padding=1), nn.BatchNorm2d(36)).eval()
    scales = 2.0 ** -(torch.arange(36, dtype=torch.float32) % 9)                      # 2^0 ... 2^-8
    with torch.no_grad():
        seq[0].weight.normal_(0, 0.25)
        seq[0].weight.view(36, -1)[:, 0] = 32 * 0.25
        seq[0].bias.zero_()
        seq[1].weight.fill_(1.0)
        seq[1].bias.zero_()
        seq[1].running_mean.zero_()
        seq[1].running_var.copy_(1.0 / scales ** 2 - 1e-5)
    conv = merge_bn(seq)[0]
    x = torch.randn(4, 32, 12, 12) * 2
    ib = int(8 - 1 - np.ceil(np.log2(float(x.abs().max()))))
    with torch.no_grad():
        ref = conv(x)
    ob = int(8 - 1 - np.ceil(np.log2(float(ref.abs().max()))))
    wb0, tb = numpy_channel_bits(conv.weight.detach().numpy())
    small = (scales <= 2.0 ** -4).nonzero().flatten()
    err = {}
    for key, wbit in (("pc", [min(b, 12 - ib + ob) for b in wb0]), ("pt", min(tb, 12 - ib + ob))):
        with torch.no_grad():
            y = run(conv, {"weight_bit": wbit, "bias_bit": ob, "input_bit": ib, "output_bit": ob}, x)
        err[key] = float(((y - ref)[:, small] ** 2).mean())
    return err["pc"] / err["pt"]


# ---- the fused block tails and the stem ------------------------------------------------------------------------------------

import test_gpu_block_tail as BT          # noqa: E402  (its cases, operands and two-launch reference)


def _rand_shift(K, centre, seed):
    rng = np.random.default_rng(seed)
    lo, hi = max(1, centre - 4), min(16, centre + 4)
    rs = rng.integers(lo, hi + 1, K).tolist()
    rs[0], rs[-1] = lo, hi
    return _shift(rs)


@pytest.mark.parametrize("case", BT.CASES, ids=lambda c: "%dx%dx%d_%dto%dto%d_%s" % (c[0], c[1], c[2], c[3], c[4], c[5], str(c[6])[-5:]))
def test_block_tail_pcs_equals_the_per_channel_launches_it_replaces(case):
    """fq_block_tail_i8_pcs against fq_conv2d_i8_add_resident_pcs + fq_conv2d_i8_resident_pcs (both checked against the oracle
    above): every output bit for bit; constant vectors give the per-tensor kernel's bytes; a per-tensor conv3 beside a
    per-channel conv1 (constant vector) as well."""
    nat = _nat()
    N, H, W, C, K3, C2, res_dtype, (ob3, g_res, ib), rs3, rs1, relu, relu1, want_wide, want_narrow = case
    x, w3, b3, res, w1, b1 = BT._operands(nat, N, H, W, C, K3, C2, res_dtype, seed=N * 1000 + K3 + C2 + 1)
    g_wide = max(0, ob3, g_res)
    rb = 2 if res_dtype == torch.int16 else 1
    v3 = _rand_shift(K3, rs3, K3 + N)
    v1 = _rand_shift(C2, rs1, C2 + N) if C2 else 0
    combos = [(v3, v1)] + ([(rs3, v1)] if C2 else [])
    for a3, a1 in combos:
        assert nat.block_tail_supported(C, K3, C2, a3, a1, ob3, g_res, rb, ib)
        nat.conv_variant_log = log = {}
        try:
            got = nat.block_tail_i8(x, w3, b3, a3, ob3, res, g_res, want_wide, g_wide, want_narrow, ib, relu, w1, b1, a1, relu1)
        finally:
            nat.conv_variant_log = None
        assert log == {"block_tail/128": 1}
        ref = BT._two_launches(nat, x, w3, b3, nat._shift_of(a3, K3, x.device), ob3, res, g_res, want_wide, g_wide, want_narrow, ib,
                               relu, w1, b1, nat._shift_of(a1, C2, x.device) if C2 else 0, relu1)
        for name, a, b in zip(("wide", "narrow", "q1"), got, ref):
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b), "%s differs in %d of %d" % (name, int((a != b).sum()), a.numel())
    const = nat.block_tail_i8(x, w3, b3, _shift([rs3] * K3), ob3, res, g_res, want_wide, g_wide, want_narrow, ib, relu, w1, b1,
                              _shift([rs1] * C2) if C2 else 0, relu1)
    pt = nat.block_tail_i8(x, w3, b3, rs3, ob3, res, g_res, want_wide, g_wide, want_narrow, ib, relu, w1, b1, rs1, relu1)
    for a, b in zip(const, pt):
        assert (a is None and b is None) or torch.equal(a, b)
    assert not nat.block_tail_supported(C, K3, C2, _shift([0] + [rs3] * (K3 - 1)), v1, ob3, g_res, rb, ib)     # integer tail only


@pytest.mark.parametrize("case", BT.PROJ_CASES, ids=lambda c: "%dx%dx%d_s%d_to%dto%d" % (c[0], c[1], c[2], c[3], c[4], c[5]))
def test_block_tail_proj_pcs_equals_the_per_channel_launches_it_replaces(case):
    """fq_block_tail_proj_i8_pcs against the projection by fq_conv2d_i8_resident_pcs followed by fq_block_tail_i8_pcs and by
    the general kernels' chain; constant vectors give the per-tensor kernel's bytes."""
    nat = _nat()
    N, H, W, sp, K3, C2, (ob3, obp, ib), rs3, rsp, rs1, relu, want_wide, want_narrow = case
    C = CP = 64
    x, w3, b3, _res, w1, b1 = BT._operands(nat, N, H, W, C, K3, C2, torch.int8, seed=N * 100 + K3 + C2 + sp + 1)
    g = torch.Generator(device="cuda").manual_seed(N * 7 + K3 + sp + 1)
    Hp, Wp = (H - 1) * sp + 1, (W - 1) * sp + 1
    xp = torch.randint(-128, 128, (N, Hp, Wp, CP), dtype=torch.int8, device="cuda", generator=g)
    wp = nat.pack_weight_krsc(torch.randint(-127, 128, (K3, CP, 1, 1), device="cuda", generator=g).float())
    bp = torch.randint(-100, 101, (K3,), device="cuda", generator=g).float()
    g_wide = max(0, ob3, obp)
    v3, vp_ = _rand_shift(K3, rs3, K3 + 1), _rand_shift(K3, rsp, K3 + 2)
    v1 = _rand_shift(C2, rs1, C2 + 3) if C2 else 0
    assert nat.block_tail_proj_supported(C, K3, C2, CP, v3, v1, vp_, sp)
    _, res = nat.conv2d_i8_resident(xp, wp, bp, (sp, sp), (0, 0), (1, 1), vp_, obp, False, True, False)
    ref = nat.block_tail_i8(x, w3, b3, v3, ob3, res, obp, want_wide, g_wide, want_narrow, ib, relu, w1, b1, v1, True)
    ref2 = BT._two_launches(nat, x, w3, b3, v3, ob3, res, obp, want_wide, g_wide, want_narrow, ib, relu, w1, b1, v1, True)
    nat.conv_variant_log = log = {}
    try:
        got = nat.block_tail_proj_i8(x, w3, b3, v3, ob3, xp, wp, bp, vp_, obp, sp, want_wide, g_wide, want_narrow, ib, relu, w1, b1, v1,
                                     True)
    finally:
        nat.conv_variant_log = None
    assert log == {"block_tail_proj/128": 1}
    for name, a, b, c in zip(("wide", "narrow", "q1"), got, ref, ref2):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b) and torch.equal(a, c), "%s differs in %d of %d" % (name, int((a != b).sum()), a.numel())
    const = nat.block_tail_proj_i8(x, w3, b3, _shift([rs3] * K3), ob3, xp, wp, bp, _shift([rsp] * K3), obp, sp, want_wide, g_wide,
                                   want_narrow, ib, relu, w1, b1, _shift([rs1] * C2) if C2 else 0, True)
    pt = nat.block_tail_proj_i8(x, w3, b3, rs3, ob3, xp, wp, bp, rsp, obp, sp, want_wide, g_wide, want_narrow, ib, relu, w1, b1, rs1,
                                True)
    for a, b in zip(const, pt):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("C,K,R,S,stride,pad,relu", [(3, 64, 7, 7, 2, 3, True), (3, 40, 3, 3, 1, 1, False), (1, 16, 5, 5, 2, 2, True),
                                                     (4, 64, 3, 3, 2, 1, False)])
def test_stem_pcs_equals_unfold_and_the_general_kernel(oracle, C, K, R, S, stride, pad, relu):
    """fq_conv2d_i8_stem_pcs (fp32 image -> int8 NHWC in one kernel) against fq_quantize_i8_unfold_w + fq_conv2d_i8_resident_pcs
    and against the oracle chain channel by channel; a constant vector gives the per-tensor kernel's bytes."""
    nat = _nat()
    rng = np.random.default_rng(C * 100 + K)
    x = (rng.standard_normal((2, C, 23, 19)) * 2).astype(np.float32)
    w = rng.integers(-128, 128, (K, C, R, S)).astype(np.int32)
    qb = np.rint(rng.standard_normal(K) * 100).astype(np.float32)
    rs = rng.integers(3, 13, K).tolist()
    rs[0], rs[-1] = 1, 16
    ib, ob = 4, 3
    rsv = _shift(rs)
    xd, qbd = torch.from_numpy(x).cuda(), torch.from_numpy(qb).cuda()
    wt = torch.from_numpy(w.astype(np.float32)).cuda()
    assert nat.stem_supported(C, K, R, S, (stride, stride), (1, 1), rsv)
    nat.conv_variant_log = log = {}
    try:
        q = nat.conv2d_i8_stem(xd, nat.pack_weight_stem(wt), qbd, K, S, (stride, stride), (pad, pad), ib, rsv, ob, relu)
    finally:
        nat.conv_variant_log = None
    assert log == {"stem/64": 1}
    cpad2 = nat.pad16(S * C)
    xu = nat.quantize_i8_unfold_w(xd, ib, S, stride, pad, 1, cpad2)
    wu = nat.pack_weight_unfold_w(wt, cpad2)
    _, ref = nat.conv2d_i8_resident(xu, wu, qbd, (stride, 1), (pad, 0), (1, 1), rsv, ob, False, True, relu)
    assert torch.equal(q, ref)
    xi = oracle.quantity(x, ib).astype(np.int32)
    acc = oracle.conv2d_int(xi, w, stride=(stride, stride), pad=(pad, pad)).astype(np.float32)
    exp = pc_epilogue(acc, qb, rs, ob) * np.float32(2.0 ** ob)
    if relu:
        exp = np.maximum(exp, 0)
    np.testing.assert_array_equal(np.moveaxis(q.cpu().numpy()[..., :K], -1, 1).astype(np.float32), exp)
    const = nat.conv2d_i8_stem(xd, nat.pack_weight_stem(wt), qbd, K, S, (stride, stride), (pad, pad), ib, _shift([7] * K), ob, relu)
    assert torch.equal(const, nat.conv2d_i8_stem(xd, nat.pack_weight_stem(wt), qbd, K, S, (stride, stride), (pad, pad), ib, 7, ob, relu))
