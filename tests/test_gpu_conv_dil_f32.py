"""fq_conv_dil_f32 -- the atrous dense 3x3 float convolution of the calibration forward, live taps only, statistic in the
epilogue -- through the C ABI, through _float_conv with FQ_OWN_DILATED=1, and inside tools.Quantity (own_dilated).  Exact agreement
with a float64 reference on integer-valued data, bit equality with the fmaf chain of include/fq.h on Gaussian data, every form of
the entry points against the plain output, and a DeepLabV3 calibration whose table does not move.    pytest -m gpu"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import cases
from conv_dil_f32_cases import IDS, SHAPES
from grouped_f32_util import _fmaf
from test_gpu_depthwise_f32 import nat  # noqa: F401  (the fixture)
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

CHUNK = 8                                                                     # FQ_CONV_DIL_F32_CHUNK
# the chain in Python: shapes of at most 2 * 10^6 fmaf calls
CHAIN = [s for s in SHAPES if s[0] * s[2] * (s[3] + 2 * s[6] - 2 * s[5]) * (s[4] + 2 * s[6] - 2 * s[5]) * 9 * s[1] <= 2_000_000]
# shapes x forms: Cout no tile multiple with batch 2, only the centre tap live, taps live for part of a tile, column blocks
FORM_SHAPES = [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[7]]
FORMS = ["null_bias", "out", "absmax", "hist", "relu", "relu_only", "act", "qd8", "qd16"]


def _chain(x, w, b, d, pad):
    """The numerics contract of fq_conv_dil_f32, literally, with libm's fmaf: one chain per output from +0.0f -- chunks of CHUNK
    input channels outermost, then the taps (r, s) ascending, then the chunk's channels ascending, a tap outside the image being
    the operand +0.0f; then acc + bias in fp32."""
    fmaf = _fmaf()
    N, C, H, W = x.shape
    K = w.shape[0]
    ho, wo = H + 2 * pad - 2 * d, W + 2 * pad - 2 * d
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    xl, wl, bias = xp.tolist(), w.tolist(), b.numpy()
    y = np.empty((N, K, ho, wo), np.float32)
    for n in range(N):
        for k in range(K):
            for p in range(ho):
                for q in range(wo):
                    acc = 0.0
                    for c0 in range(0, C, CHUNK):
                        for r in range(3):
                            for s in range(3):
                                for c in range(c0, c0 + CHUNK):
                                    acc = fmaf(wl[k][c][r][s], xl[n][c][p + r * d][q + s * d], acc)
                    y[n, k, p, q] = np.float32(acc) + bias[k]
    return torch.from_numpy(y)


_CASES = {}


def _case(shape, integer):
    """(x, w, the packed weights, b on the GPU, the kernel's plain output) of a shape, computed once and shared."""
    key = (shape, integer)
    if key not in _CASES:
        from common.quantity import _native
        N, C, K, H, W, d, pad = shape
        g = torch.Generator().manual_seed(1000 * sum(shape) + integer)
        if integer:                                                           # |sum| <= 9 Cin 32 + 100 < 2^24: exact in any order
            assert 9 * C * 32 + 100 < 2 ** 24
            x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
            w = torch.randint(-4, 5, (K, C, 3, 3), generator=g).float()
            b = torch.randint(-100, 101, (K,), generator=g).float()
        else:
            x, w, b = torch.randn(N, C, H, W, generator=g), torch.randn(K, C, 3, 3, generator=g) / 3, torch.randn(K, generator=g)
        x, w, b = x.cuda(), w.cuda(), b.cuda()
        wq = _native.pack_kxk_weight(w)
        _CASES[key] = (x, w, wq, b, _native.conv_dil_f32(x, wq, b, d, pad))
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_valued_data(nat, shape):
    x, w, _, b, y = _case(shape, True)
    ref = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=shape[6], dilation=shape[5])
    assert y.shape == ref.shape and torch.equal(y.double().cpu(), ref)


@pytest.mark.parametrize("shape", CHAIN, ids=["x".join(map(str, s)) for s in CHAIN])
def test_gaussian_data_has_the_bits_of_the_fmaf_chain(nat, shape):
    x, w, _, b, y = _case(shape, False)
    want = _chain(x.cpu(), w.cpu(), b.cpu(), shape[5], shape[6])
    assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", [s for s in CHAIN if s[0] > 1], ids=["x".join(map(str, s)) for s in CHAIN if s[0] > 1])
def test_image_one_of_a_batch_has_the_bits_of_that_image_alone(nat, shape):
    x, _, wq, b, y = _case(shape, False)
    alone = nat.conv_dil_f32(x[1:2].contiguous(), wq, b, shape[5], shape[6])
    assert torch.equal(alone[0].view(torch.int32), y[1].view(torch.int32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", FORM_SHAPES, ids=["x".join(map(str, s)) for s in FORM_SHAPES])
def test_every_form_stores_the_bits_of_the_plain_one(nat, oracle, shape, form):
    x, _, wq, b, y = _case(shape, False)
    d, pad = shape[5], shape[6]
    run = lambda **kw: nat.conv_dil_f32(x, wq, b, d, pad, **kw)
    amax = float(y.abs().max())
    if form == "null_bias":
        zero = nat.conv_dil_f32(x, wq, torch.zeros_like(b), d, pad)
        assert torch.equal(nat.conv_dil_f32(x, wq, None, d, pad).view(torch.int32), zero.view(torch.int32))
    elif form == "out":                                                       # a view at an odd float offset, between sentinels
        buf = torch.full((y.numel() + 8,), 777.0, device="cuda")
        out = buf[3:3 + y.numel()].view(y.shape)
        assert run(out=out) is out and torch.equal(out, y)
        assert bool((buf[:3] == 777.0).all()) and bool((buf[3 + y.numel():] == 777.0).all())
    elif form == "absmax":
        mx = torch.tensor([0.0, 0.0, 1e9], device="cuda")
        assert torch.equal(run(max_dev=mx, row=1), y) and mx.tolist() == [0.0, amax, 1e9]
    elif form == "hist":
        iv = torch.tensor([1.0, amax / 2048 + 1e-12, 1.0], device="cuda")
        hist = torch.zeros(3, 2048, dtype=torch.int64, device="cuda")
        assert torch.equal(run(interval_dev=iv, hist_dev=hist, row=1), y)
        want = oracle.hist2048(y.cpu().numpy(), float(iv[1]))
        assert np.array_equal(hist[1].cpu().numpy(), want) and int(hist[0].sum()) == 0 and int(hist[2].sum()) == 0
        assert int(want.sum()) == int((y != 0).sum())
    elif form == "relu":
        r = torch.full_like(y, -7.0)
        assert torch.equal(run(relu_out=r), y) and torch.equal(r, torch.relu(y))
    elif form == "relu_only":                                                 # y is not written; the statistic is still y's
        r, mx = torch.full_like(y, -7.0), torch.zeros(1, device="cuda")
        assert run(max_dev=mx, row=0, relu_out=r, out=False) is None
        assert torch.equal(r, torch.relu(y)) and float(mx[0]) == amax
    elif form == "act":
        r, mx = torch.full_like(y, -7.0), torch.zeros(1, device="cuda")
        assert torch.equal(run(max_dev=mx, row=0, relu_out=r, act=6.0), y)
        assert torch.equal(r, torch.nn.functional.relu6(y)) and float(mx[0]) == amax
        y6 = nat.conv_dil_f32(x * 8, wq, b, d, pad)                           # ... and on values that reach the cap
        r6 = torch.empty_like(y6)
        nat.conv_dil_f32(x * 8, wq, b, d, pad, relu_out=r6, act=6.0, out=False)
        assert torch.equal(r6, torch.nn.functional.relu6(y6)) and float(r6.max()) == 6.0
    else:
        bit, bw = (4, 8) if form == "qd8" else (9, 16)
        assert torch.equal(run(qd=(bit, bw)), nat.quandequan(y, bit, bw))


def test_float_conv_takes_atrous_dense_layers_with_the_switch_on(nat, monkeypatch):
    from common.quantity import _float_conv
    conv = nn.Conv2d(32, 20, 3, padding=6, dilation=6).cuda().eval()
    x = torch.randn(3, 32, 14, 14, device="cuda")
    monkeypatch.delenv("FQ_OWN_DILATED", raising=False)
    assert _float_conv.kind(conv, x) is None
    monkeypatch.setenv("FQ_OWN_DILATED", "1")
    assert _float_conv.kind(conv, x) == "kd" and _float_conv.kind(conv, x, dilated=False) is None
    own = nat.conv_dil_f32(x, nat.pack_kxk_weight(conv.weight), conv.bias.detach(), 6, 6)
    with torch.no_grad():
        out = _float_conv.call(conv, x)
        assert torch.equal(out, own) and _float_conv.is_verified(conv, "kd") and not _float_conv.is_off(conv)
        assert torch.equal(_float_conv.call_qd(conv, x, 4, 8), nat.quandequan(own, 4))


def test_deeplabv3_calibration_with_the_kernel(nat):
    """DeepLabV3 at output stride 16, width 16, on 64 x 64 (4 x 4 atrous planes), BatchNorm merged, sparse integer
    parameters: every partial sum of every convolution is an integer below 2^24 and exact in any order, so the table must be
    byte-identical with own_dilated on and off."""
    from common.quantity import _float_conv, merge_bn
    from model.deeplab.DeepLabV3_fabu import DeepLabV3
    from tools import Quantity
    model = merge_bn(cases.seed_model(DeepLabV3(num_classes=5, output_stride=16, width=16, input_size=64)).eval())
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 4:                                                  # one weight of +-1 per output channel: a block at
                flat = torch.zeros(p.shape[0], p[0].numel())                  # most doubles |x| + 3, sixteen blocks stay below 2^24
                at = torch.randint(0, p[0].numel(), (p.shape[0], 1), generator=g)
                flat.scatter_(1, at, torch.randint(0, 2, (p.shape[0], 1), generator=g).float() * 2 - 1)
                p.copy_(flat.view(p.shape))
            else:
                p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    model = model.cuda()
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randint(-2, 3, (2, 3, 64, 64), generator=g).float(), torch.zeros(2, dtype=torch.long)) for _ in range(3)]
    dilated = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups == 1 and m.dilation[0] > 1]
    assert len(dilated) == 5                                                  # two 3x3s of layer4, three ASPP branches
    absnet, peak = copy.deepcopy(model).double(), [0.0]                       # the bound: |parameters| on |images| in float64
    with torch.no_grad():
        for p in absnet.parameters():
            p.abs_()
        for m in absnet.modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, i, o: peak.__setitem__(0, max(peak[0], float(o.abs().max()))))
        for images, _ in batches:
            absnet(images.cuda().double().abs())
    assert 0 < peak[0] < 2 ** 24, peak
    runs = []
    # (the first calibration of a model proves its conv -> add chains on its first batch and launches their thirteen 1x1
    #  convolutions unchained there: it is run, and only the two behind it are compared)
    for own in (False, True, False):
        with product_workdir(input_shape="1,3,64,64", device="gpu", max_cali_img_num=1) as tmp:
            q = Quantity(model)
            q.own_dilated = own
            q.activation_quantize(batches)
            runs.append((open(tmp + "/test/workdir/feat.table", "rb").read(), q.timings["own_conv1x1_launches"]))
        if own:
            assert all(_float_conv.is_verified(m, "kd") and not _float_conv.is_off(m) for m in dilated)
    (on, n_on), (off, n_off) = runs[1:]
    assert runs[0][0] == off
    assert len(on) > 0 and on == off
    assert n_on - n_off == 2 * len(dilated), (n_on, n_off)                    # the dilated layers x the two pass-1 batches
