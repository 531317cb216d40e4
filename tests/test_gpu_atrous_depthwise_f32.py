"""fq_dwconv_dil_f32 -- the atrous depthwise float convolution of the calibration forward, statistic in the epilogue -- through
the C ABI, through _float_conv with FQ_OWN_ATROUS=1, and inside tools.Quantity (own_atrous).  Exact agreement with a float64
reference on integer-valued data, bit equality with the fmaf chain of include/fq.h on Gaussian data, every form of the entry
points against the plain output, and a DeepLabV3+ calibration whose table does not move.    pytest -m gpu"""
import numpy as np
import pytest
import torch
from torch import nn

import cases
from atrous_f32_cases import IDS, SHAPES
from grouped_f32_util import _fmaf
from test_gpu_depthwise_f32 import nat  # noqa: F401  (the fixture)
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

# shapes x forms: odd rows, only the centre tap inside, 5x5, more planes than a tile, row bands with column blocks
FORM_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[9], SHAPES[12]]
FORMS = ["null_bias", "out", "absmax", "hist", "relu", "relu_only", "act", "qd8", "qd16"]


def _ref64(x, w, b, d, pad):
    """float64 F.conv2d(groups=C, dilation=d) on the host."""
    return torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), padding=pad,
                                      dilation=d, groups=x.shape[1])


def _chain(x, w, b, d, pad):
    """The numerics contract of fq_dwconv_dil_f32, literally, with libm's fmaf: one chain per output from +0.0f, r outer, s
    inner, a tap outside the image being the operand +0.0f; then acc + bias in fp32."""
    fmaf = _fmaf()
    N, C, H, W = x.shape
    R = w.shape[2]
    ho, wo = H + 2 * pad - d * (R - 1), W + 2 * pad - d * (R - 1)
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    xl, wl, bias = xp.tolist(), w.tolist(), b.numpy()
    y = np.empty((N, C, ho, wo), np.float32)
    for n in range(N):
        for c in range(C):
            plane, wc = xl[n][c], wl[c][0]
            for p in range(ho):
                for q in range(wo):
                    acc = 0.0
                    for r in range(R):
                        row = plane[p + r * d]
                        for s in range(R):
                            acc = fmaf(wc[r][s], row[q + s * d], acc)
                    y[n, c, p, q] = np.float32(acc) + bias[c]
    return torch.from_numpy(y)


_CASES = {}


def _case(shape, integer):
    """(x, w, b on the GPU, the kernel's plain output) of a shape, computed once and shared."""
    key = (shape, integer)
    if key not in _CASES:
        N, C, H, W, R, d, pad = shape
        g = torch.Generator().manual_seed(1000 * sum(shape) + integer)
        if integer:                                                           # |sum| <= 25 * 8 * 4 + 100: exact in any order
            x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
            w = torch.randint(-4, 5, (C, 1, R, R), generator=g).float()
            b = torch.randint(-100, 101, (C,), generator=g).float()
        else:
            x, w, b = torch.randn(N, C, H, W, generator=g), torch.randn(C, 1, R, R, generator=g) / R, torch.randn(C, generator=g)
        x, w, b = x.cuda(), w.cuda(), b.cuda()
        from common.quantity import _native
        _CASES[key] = (x, w, b, _native.dwconv_dil_f32(x, w, b, (R, R), d, pad))
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_valued_data(nat, shape):
    x, w, b, y = _case(shape, True)
    ref = _ref64(x, w, b, shape[5], shape[6])
    assert y.shape == ref.shape and torch.equal(y.double().cpu(), ref)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gaussian_data_has_the_bits_of_the_fmaf_chain(nat, shape):
    x, w, b, y = _case(shape, False)
    want = _chain(x.cpu(), w.cpu(), b.cpu(), shape[5], shape[6])
    assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1], ids=[i for s, i in zip(SHAPES, IDS) if s[0] > 1])
def test_image_one_of_a_batch_has_the_bits_of_that_image_alone(nat, shape):
    x, w, b, y = _case(shape, False)
    alone = nat.dwconv_dil_f32(x[1:2].contiguous(), w, b, (shape[4],) * 2, shape[5], shape[6])
    assert torch.equal(alone[0].view(torch.int32), y[1].view(torch.int32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", FORM_SHAPES, ids=["x".join(map(str, s)) for s in FORM_SHAPES])
def test_every_form_stores_the_bits_of_the_plain_one(nat, oracle, shape, form):
    x, w, b, y = _case(shape, False)
    k, d, pad = (shape[4],) * 2, shape[5], shape[6]
    run = lambda **kw: nat.dwconv_dil_f32(x, w, b, k, d, pad, **kw)
    amax = float(y.abs().max())
    if form == "null_bias":
        zero = nat.dwconv_dil_f32(x, w, torch.zeros_like(b), k, d, pad)
        assert torch.equal(nat.dwconv_dil_f32(x, w, None, k, d, pad).view(torch.int32), zero.view(torch.int32))
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
        y6 = nat.dwconv_dil_f32(x * 8, w, b, k, d, pad)                       # ... and on values that reach the cap
        r6 = torch.empty_like(y6)
        nat.dwconv_dil_f32(x * 8, w, b, k, d, pad, relu_out=r6, act=6.0, out=False)
        assert torch.equal(r6, torch.nn.functional.relu6(y6)) and float(r6.max()) == 6.0
    else:
        bit, bw = (4, 8) if form == "qd8" else (9, 16)
        assert torch.equal(run(qd=(bit, bw)), nat.quandequan(y, bit, bw))


def test_float_conv_takes_atrous_depthwise_layers_with_the_switch_on(nat, monkeypatch):
    from common.quantity import _float_conv
    conv = nn.Conv2d(20, 20, 3, padding=6, dilation=6, groups=20).cuda().eval()
    x = torch.randn(3, 20, 14, 14, device="cuda")
    monkeypatch.delenv("FQ_OWN_ATROUS", raising=False)
    assert _float_conv.kind(conv, x) is None
    monkeypatch.setenv("FQ_OWN_ATROUS", "1")
    assert _float_conv.kind(conv, x) == "dwd" and _float_conv.kind(conv, x, atrous=False) is None
    assert _float_conv.weight(conv, "dwd").data_ptr() == conv.weight.data_ptr()
    own = nat.dwconv_dil_f32(x, conv.weight.detach(), conv.bias.detach(), (3, 3), 6, 6)
    with torch.no_grad():
        out = _float_conv.call(conv, x)
        assert torch.equal(out, own) and _float_conv.is_verified(conv, "dwd") and not _float_conv.is_off(conv)
        assert torch.equal(_float_conv.call_qd(conv, x, 4, 8), nat.quandequan(own, 4))


def _deeplab(integer):
    """DeepLabV3+ at output stride 16 on 64 x 64 (4 x 4 atrous planes), BatchNorm merged.  integer: small sparse integer
    parameters, so that every partial sum of every convolution is an integer below 2^24 and exact in any order."""
    from common.quantity import merge_bn
    from model.deeplab.DeepLabV3Plus_fabu import DeepLabV3Plus
    model = merge_bn(cases.seed_model(DeepLabV3Plus(num_classes=5, output_stride=16, width_mult=0.25, input_size=64)).eval())
    if integer:
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() == 4:                                              # +-1 or 0: about four non-zero weights per output
                    keep = 4.0 / max(p[0].numel(), 4)
                    p.copy_((torch.randint(0, 2, p.shape, generator=g).float() * 2 - 1) * (torch.rand(p.shape, generator=g) < keep).float())
                else:
                    p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    return model.cuda()


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "gaussian"])
def test_deeplab_calibration_with_the_kernel(nat, integer, capsys):
    from common.quantity import _float_conv
    from tools import Quantity
    model = _deeplab(integer)
    g = torch.Generator().manual_seed(21)
    batches = ([(torch.randint(-2, 3, (2, 3, 64, 64), generator=g).float(), torch.zeros(2, dtype=torch.long)) for _ in range(3)]
               if integer else cases.calib_batches(3, (2, 3, 64, 64), seed=31))
    atrous = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1 and m.dilation[0] > 1]
    assert len(atrous) == 7
    if integer:                                                               # the bound: |parameters| on |images| in float64
        import copy
        absnet, peak = copy.deepcopy(model).double(), [0.0]
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
    for own in (True, False):
        with product_workdir(input_shape="1,3,64,64", device="gpu", max_cali_img_num=1) as tmp:
            q = Quantity(model)
            q.own_depthwise, q.fuse_relu6, q.own_atrous = True, True, own
            q.activation_quantize(batches)
            runs.append((open(tmp + "/test/workdir/feat.table", "rb").read(), q.timings["own_conv1x1_launches"]))
        if own:
            assert all(_float_conv.is_verified(m, "dwd") and not _float_conv.is_off(m) for m in atrous)
    (on, n_on), (off, n_off) = runs
    assert len(on) > 0
    if integer:
        assert on == off
        # the atrous layers x the two pass-1 batches (batches 0 .. MAX_CALI_IMG_NUM).  (Not on Gaussian data: there the library
        # arm may switch its bias fusion off for the run when the library's convolution with and without bias differ in a bit.)
        assert n_on - n_off == 2 * len(atrous), (n_on, n_off)
    else:
        rows_on, rows_off = on.splitlines(), off.splitlines()
        assert len(rows_on) == len(rows_off)
        with capsys.disabled():
            print("\n[atrous depthwise f32] DeepLabV3+ os16 64x64: %d of %d feat.table rows differ between own_atrous on and off"
                  % (sum(a != b for a, b in zip(rows_on, rows_off)), len(rows_on)))
