"""fq_dwconv_f32 -- the depthwise float convolution of the calibration forward, statistic in the epilogue -- through the C ABI,
through _float_conv with FQ_OWN_DWCONV=1, and inside tools.Quantity (own_depthwise).  Exact agreement with a float64 reference on
integer-valued data (every partial sum is exact, so an indexing or tiling mistake shows as a wrong bit), the project's
summation-order bound on Gaussian data, the four forms of the entry point bit for bit against each other, padding that leaks
nothing, return codes, and calibrations whose tables do not move.    pytest -m gpu"""
import copy

import pytest
import torch
from torch import nn

import cases
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

# N, C, H, W, R, stride, pad: a single pixel, a 1x1 output, pad = R - 1, odd planes, a row wider and a plane taller than any tile,
# planes packed into one tile, more planes than one pass of the grid packs
SHAPES = [(1, 1, 1, 1, 3, 1, 1), (2, 3, 3, 3, 3, 1, 0), (1, 5, 4, 6, 5, 1, 4), (3, 7, 7, 7, 3, 1, 1), (2, 19, 14, 14, 3, 2, 1),
          (2, 4, 13, 9, 5, 2, 2), (1, 3, 17, 23, 3, 2, 0), (1, 2, 56, 56, 3, 1, 1), (1, 2, 112, 112, 3, 2, 1), (1, 1, 5, 300, 3, 1, 1),
          (1, 1, 300, 5, 5, 1, 2), (2, 67, 7, 7, 5, 1, 2), (64, 32, 7, 7, 3, 1, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from common.quantity import _native
    _native.lib()
    return _native


def _ref64(x, w, b, stride, pad):
    """float64 F.conv2d(groups=C) on the host (x, w, b: any device); returned on the GPU."""
    y = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), stride=stride,
                                   padding=pad, groups=x.shape[1])
    return y.cuda()


_CASES = {}


def _case(shape, integer):
    """(x, w, b, float64 reference, float64 bound, the kernel's plain output) of a shape, computed once and shared."""
    key = (shape, integer)
    if key not in _CASES:
        N, C, H, W, R, stride, pad = shape
        g = torch.Generator().manual_seed(1000 * sum(shape) + integer)
        if integer:                                                           # |sum| <= 25 * 8 * 4 + 100: exact in any order
            x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
            w = torch.randint(-4, 5, (C, 1, R, R), generator=g).float()
            b = torch.randint(-100, 101, (C,), generator=g).float()
        else:
            x, w, b = torch.randn(N, C, H, W, generator=g), torch.randn(C, 1, R, R, generator=g) / R, torch.randn(C, generator=g)
        x, w, b = x.cuda(), w.cuda(), b.cuda()
        from common.quantity import _native
        _CASES[key] = (x, w, b, _ref64(x, w, b, stride, pad), _ref64(x.abs(), w.abs(), b.abs(), stride, pad),
                       _native.dwconv_f32(x, w, b, (R, R), stride, pad))
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_valued_data(nat, shape):
    x, w, b, ref, _bound, y = _case(shape, True)
    R, stride, pad = shape[4:]
    assert y.shape == ref.shape and torch.equal(y.double(), ref)
    assert torch.equal(nat.dwconv_f32(x, w, None, (R, R), stride, pad).double(), _ref64(x, w, None, stride, pad))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gaussian_data_within_the_bound_repeatable_and_independent_of_the_batch(nat, shape):
    from common.quantity import _float_conv
    x, w, b, ref, bound, y = _case(shape, False)
    R, stride, pad = shape[4:]
    assert bool(((y.double() - ref).abs() <= _float_conv.TOL * bound).all())
    assert torch.equal(nat.dwconv_f32(x, w, b, (R, R), stride, pad), y)              # same bits from run to run
    for i in sorted({0, x.shape[0] // 2, x.shape[0] - 1}) if x.shape[0] > 1 else ():
        assert torch.equal(nat.dwconv_f32(x[i:i + 1].contiguous(), w, b, (R, R), stride, pad)[0], y[i]), i


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_four_forms_store_the_same_bits(nat, shape):
    x, w, b, _ref, _bound, y = _case(shape, False)
    R, stride, pad = shape[4:]
    k = (R, R)
    amax = float(y.abs().max())
    # pass 1: the abs-max folded into an existing maximum, the ReLU copy
    mx = torch.tensor([0.0, 1e9, 0.0], device="cuda")
    r = torch.full_like(y, -7.0)
    y1 = nat.dwconv_f32(x, w, b, k, stride, pad, max_dev=mx, row=2, relu_out=r)
    assert torch.equal(y1, y) and torch.equal(r, torch.clamp_min(y, 0))
    assert mx.tolist() == [0.0, 1e9, amax]
    nat.dwconv_f32(x, w, b, k, stride, pad, max_dev=mx, row=1)
    assert float(mx[1]) == 1e9                                                       # a larger running maximum stays
    # pass 2: the histogram, accumulated onto existing counts, against the streaming kernel on the plain output; the last two
    # intervals lie outside the fast-quotient range (IEEE divide: everything in the last / first bin)
    for ivv in (amax / 2048 + 1e-12, 1e-30, 3e25):
        iv = torch.tensor([1.0, ivv], device="cuda")
        hist = torch.zeros(2, 2048, dtype=torch.int64, device="cuda")
        hist[1, 5] = 7
        want = hist.clone()
        y2 = nat.dwconv_f32(x, w, b, k, stride, pad, interval_dev=iv, hist_dev=hist, row=1)
        nat.hist2048_seg([y], [1], iv, want)
        assert torch.equal(y2, y) and torch.equal(hist, want), ivv
        assert int(hist[1].sum()) - 7 == int((y != 0).sum()) and int(hist[0].sum()) == 0
    # only the ReLU's output wanted: y's allocation is not touched, the statistic is still that of y
    sentinel = torch.full_like(y, 12345.0)
    mx2 = torch.zeros(1, device="cuda")
    r2 = torch.full_like(y, -7.0)
    assert nat.dwconv_f32(x, w, b, k, stride, pad, max_dev=mx2, row=0, relu_out=r2, out=False) is None
    assert torch.equal(r2, torch.clamp_min(y, 0)) and float(mx2[0]) == amax and bool((sentinel == 12345.0).all())
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    iv = torch.tensor([amax / 2048 + 1e-12], device="cuda")
    r2.fill_(-7.0)
    nat.dwconv_f32(x, w, b, k, stride, pad, interval_dev=iv, hist_dev=hist, row=0, relu_out=r2, out=False)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want) and torch.equal(r2, torch.clamp_min(y, 0)) and bool((sentinel == 12345.0).all())
    # TestConv's form: QuanDequan of the plain output
    for bit, bw in ((4, 8), (-1, 8), (9, 16)):
        assert torch.equal(nat.dwconv_f32(x, w, b, k, stride, pad, qd=(bit, bw)), nat.quandequan(y, bit, bw)), (bit, bw)


def test_nan_and_zero_outputs(nat):
    shape = (2, 6, 9, 11, 3, 1, 1)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, shape[:4], generator=g).float().cuda()
    w = torch.randint(-4, 5, (6, 1, 3, 3), generator=g).float().cuda()
    w[w == 0] = 1.0                                                                  # (every window that covers a NaN is NaN either way: 0 * NaN)
    w[2] = 0.0                                                                       # exactly-zero outputs: a whole channel
    b = torch.zeros(6, device="cuda")
    x[1, 4, 3, 5] = float("nan")
    x[0, 0, 8, 10] = float("nan")                                                    # a corner: its window is cut by the padding
    ref = _ref64(x, w, b, 1, 1)
    mx = torch.zeros(1, device="cuda")
    r = torch.empty(2, 6, 9, 11, device="cuda")
    y = nat.dwconv_f32(x, w, b, (3, 3), 1, 1, max_dev=mx, row=0, relu_out=r)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and int(torch.isnan(y).sum()) == 9 + 4
    assert torch.equal(torch.isnan(r), torch.isnan(ref))
    assert torch.equal(y[~torch.isnan(y)].double(), ref[~torch.isnan(ref)]) and bool((y[:, 2] == 0).all())
    assert float(mx[0]) == float(y[~torch.isnan(y)].abs().max())                    # NaN does not enter the maximum
    iv = torch.tensor([float(mx[0]) / 2048 + 1e-12], device="cuda")
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    nat.dwconv_f32(x, w, b, (3, 3), 1, 1, interval_dev=iv, hist_dev=hist, row=0)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want)
    assert int(hist.sum()) <= int((y != 0).sum())                                    # exact zeros are not counted


@pytest.mark.parametrize("R,stride,pad", [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (5, 1, 2), (5, 2, 2)])
def test_no_value_leaks_through_the_padding(nat, R, stride, pad):
    """+Inf at the last element of plane p and at the first element of plane p + 1: the padded taps next to them must be the
    operand 0, never the neighbouring plane's (or row's) element -- an Inf that leaked would make a finite output non-finite,
    and 0 * Inf a NaN.  The output is a view between sentinel floats, at an odd float offset."""
    from common.quantity import _float_conv
    N, C, H, W = 2, 5, 9, 7
    g = torch.Generator().manual_seed(R * 10 + stride + pad)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    w = (torch.randn(C, 1, R, R, generator=g).abs() + 0.1).cuda()
    b = torch.randn(C, generator=g).cuda()
    for p in (1, 4, 7):                                                              # plane 4 -> 5 crosses the image boundary
        x.view(N * C, H, W)[p, H - 1, W - 1] = float("inf")
        x.view(N * C, H, W)[p + 1, 0, 0] = float("inf")
    ref = _ref64(x, w, b, stride, pad)
    finite = torch.isfinite(ref)
    assert bool(finite.any()) and not bool(finite.all())
    xf = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    bound = _ref64(xf.abs(), w.abs(), b.abs(), stride, pad)
    buf = torch.full((ref.numel() + 8,), 777.0, device="cuda")
    y = buf[3:3 + ref.numel()].view(ref.shape)
    assert y.data_ptr() % 16 != 0
    nat.dwconv_f32(x, w, b, (R, R), stride, pad, out=y)
    assert bool((buf[:3] == 777.0).all()) and bool((buf[3 + ref.numel():] == 777.0).all())
    assert torch.equal(torch.isfinite(y), finite)
    assert bool(((y.double() - ref).abs()[finite] <= _float_conv.TOL * bound[finite]).all())


def test_return_codes(nat):
    L = nat.lib()
    x = torch.zeros(2, 4, 6, 6, device="cuda")
    w = torch.zeros(4, 1, 5, 5, device="cuda")
    b = torch.zeros(4, device="cuda")
    y = torch.zeros(2, 4, 16, 16, device="cuda")                                    # room for every geometry below
    one = torch.zeros(2, device="cuda")
    h = torch.zeros(2048, dtype=torch.int64, device="cuda")
    X, Wp, B, Y = x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr()

    def call(xp=X, wp=Wp, bp=B, yp=Y, rp=None, N=2, C=4, H=6, W=6, R=3, S=3, stride=1, pad=1, mp=None, ip=None, hp=None):
        return L.fq_dwconv_f32(xp, wp, bp, yp, rp, N, C, H, W, R, S, stride, pad, mp, ip, hp, None)

    assert call() == 0 and call(bp=None) == 0 and call(yp=None, rp=Y) == 0
    # geometries the kernel declines: FQ_ERR_UNSUPPORTED, and fq_dwconv_f32_supported says so too
    geoms = [(dict(), True), (dict(R=5, S=5, pad=4), True), (dict(stride=2, pad=0), True), (dict(H=1, W=1), True),
             (dict(R=7, S=7, pad=3), False), (dict(R=1, S=1, pad=0), False), (dict(R=3, S=5), False), (dict(stride=3), False),
             (dict(pad=3), False), (dict(R=5, S=5, pad=5), False), (dict(H=2, pad=0), False), (dict(W=1, pad=0), False)]
    for kw, ok in geoms:
        rc = call(**kw)
        assert rc == (0 if ok else -4), (kw, rc)
        a = dict(C=4, R=3, S=3, stride=1, pad=1, H=6, W=6)
        a.update({k: v for k, v in kw.items() if k in a})
        assert L.fq_dwconv_f32_supported(a["C"], a["R"], a["S"], a["stride"], a["stride"], a["pad"], a["pad"], 1, 1, a["H"], a["W"]) == int(ok)
    assert L.fq_dwconv_f32_supported(4, 3, 3, 1, 1, 1, 1, 2, 2, 6, 6) == 0           # dilation
    assert L.fq_dwconv_f32_supported(4, 3, 3, 1, 2, 1, 1, 1, 1, 6, 6) == 0           # stride (1, 2)
    assert L.fq_dwconv_f32_supported(4, 3, 3, 1, 1, 1, 2, 1, 1, 6, 6) == 0           # padding (1, 2)
    assert L.fq_dwconv_f32_supported(0, 3, 3, 1, 1, 1, 1, 1, 1, 6, 6) == 0
    assert call(N=1 << 14, C=1 << 10, H=8, W=8) == -4                                # 2^30 elements
    # invalid arguments: FQ_ERR_INVALID_ARG
    for kw in (dict(xp=None), dict(wp=None), dict(yp=None), dict(xp=X + 2), dict(wp=Wp + 1), dict(yp=Y + 2), dict(bp=B + 2),
               dict(rp=Y + 1), dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(N=-1), dict(stride=0), dict(pad=-1), dict(R=0, S=0),
               dict(mp=one.data_ptr(), ip=one.data_ptr(), hp=h.data_ptr()), dict(hp=h.data_ptr()), dict(mp=one.data_ptr() + 2),
               dict(ip=one.data_ptr(), hp=h.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    qd = lambda bit, bw, yp=Y: L.fq_dwconv_qd_f32(X, Wp, B, yp, 2, 4, 6, 6, 3, 3, 1, 1, bit, bw, None)
    assert qd(4, 8) == 0 and qd(4, 7) == -1 and qd(121, 8) == -1 and qd(4, 8, None) == -1
    assert L.fq_dwconv_qd_f32(X, Wp, B, Y, 2, 4, 6, 6, 7, 7, 1, 3, 4, 8, None) == -4
    torch.cuda.synchronize()
    with pytest.raises(nat.FqError):
        nat.dwconv_f32(x, torch.zeros(4, 1, 7, 7, device="cuda"), b, (7, 7), 1, 3)


def test_float_conv_takes_depthwise_layers_with_the_switch_on(nat, monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.setenv("FQ_OWN_DWCONV", "1")
    conv = nn.Conv2d(19, 19, 3, stride=2, padding=1, groups=19).cuda().eval()
    x = torch.randn(3, 19, 14, 14, device="cuda")
    assert _float_conv.kind(conv, x) == "dw" and _float_conv.kind(conv, x, depthwise=False) is None
    assert _float_conv.weight(conv, "dw").data_ptr() == conv.weight.data_ptr()
    own = nat.dwconv_f32(x, conv.weight.detach(), conv.bias.detach(), (3, 3), 2, 1)
    seen = []
    handle = conv.register_forward_hook(lambda m, i, o: seen.append(o))
    with torch.no_grad():
        out = _float_conv.call(conv, x)
        assert len(seen) == 1 and seen[0] is out and torch.equal(out, own)           # the kernel's tensor; hooks fire
        assert _float_conv.is_verified(conv, "dw") and not _float_conv.is_off(conv) and "forward" not in conv.__dict__
        assert _float_conv.call_qd(conv, x, 4, 8) is None                             # somebody watches the un-quantised output
        handle.remove()
        calls, real = [], nat.dwconv_f32
        monkeypatch.setattr(nat, "dwconv_f32", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
        fused = _float_conv.call_qd(conv, x, 4, 8)
        assert len(calls) == 1 and calls[0] == {"qd": (4, 8)} and torch.equal(fused, nat.quandequan(own, 4))
        monkeypatch.setattr(nat, "dwconv_f32", real)
        # a module that disagrees keeps the library convolution
        other = copy.deepcopy(conv)
        monkeypatch.setattr(_float_conv, "TOL", -1.0)
        lib_out = _float_conv.call(other, x)
        assert _float_conv.is_off(other) and not _float_conv.is_verified(other, "dw") and _float_conv.kind(other, x) is None
        assert torch.equal(lib_out, nn.Conv2d.forward(other, x))
        monkeypatch.setattr(_float_conv, "TOL", 1e-5)
        assert float((lib_out - own).abs().max()) <= 1e-4
        # declined layers stay None with the switch on; with it off so does this one
        assert _float_conv.kind(nn.Conv2d(16, 16, 3, padding=1, groups=4).cuda(), torch.zeros(1, 16, 8, 8, device="cuda")) is None
        assert _float_conv.kind(nn.Conv2d(16, 32, 3, padding=1, groups=16).cuda(), torch.zeros(1, 16, 8, 8, device="cuda")) is None
        monkeypatch.setenv("FQ_OWN_DWCONV", "0")
        assert _float_conv.kind(conv, x) is None


def _integer_separable_net():
    """tests/golden/cases.py's tiny separable net with small sparse integer parameters: every partial sum of every convolution is
    an integer below 2^24, so every fp32 sum is exact whatever its order."""
    model = cases.tiny_separable_net().eval()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 4:
                keep = 0.5 if p.shape[1] <= 3 or p.shape[2] > 1 else 0.25
                v = torch.randint(0, 2, p.shape, generator=g).float() * 2 - 1
                p.copy_(v * (torch.rand(p.shape, generator=g) < keep).float())
            elif p.dim() == 2:
                p.copy_(torch.randint(-1, 2, p.shape, generator=g).float() * (torch.rand(p.shape, generator=g) < 0.125).float())
            else:
                p.copy_(torch.randint(-3, 4, p.shape, generator=g).float())
    return model


def test_calibration_with_the_kernel_is_byte_identical_on_exact_data():
    from common.quantity import _float_conv
    from tools import Quantity
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randint(-2, 3, (4, 3, 16, 16), generator=g).float(), torch.zeros(4, dtype=torch.long)) for _ in range(5)]
    # the bound, on the host in float64: the forward of |parameters| on |images| dominates every partial sum of every layer
    absnet = copy.deepcopy(_integer_separable_net()).double()
    with torch.no_grad():
        for p in absnet.parameters():
            p.abs_()
    peak, hooks = [0.0], []
    for m in absnet.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            hooks.append(m.register_forward_hook(lambda mod, i, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))))
    with torch.no_grad():
        for images, _ in batches:
            absnet(images.double().abs())
    assert 0 < peak[0] < 2 ** 24, peak
    runs = []
    for own in (True, False):
        with product_workdir(input_shape="1,3,16,16", device="gpu", max_cali_img_num=3) as tmp:
            q = Quantity(_integer_separable_net().cuda())
            q.own_depthwise = own
            bits = q.activation_quantize(batches)
            runs.append((dict(bits), open(tmp + "/test/workdir/feat.table", "rb").read(), dict(q._collector.max_vals),
                         q._collector.hist_device.clone(), q.timings["own_conv1x1_launches"]))
            dws = [q.model.dw1, q.model.dw2, q.model.dw3]
            if own:
                assert all(_float_conv.is_verified(m, "dw") and not _float_conv.is_off(m) for m in dws)
            else:
                assert not any(_float_conv.is_verified(m) for m in dws)
    on, off = runs
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and torch.equal(on[3], off[3])
    assert int(on[3].sum()) > 0
    assert on[4] - off[4] == 3 * 4, (on[4], off[4])         # three depthwise layers x pass-1 batches (batches 0 .. MAX_CALI_IMG_NUM)


@pytest.mark.parametrize("residual,hw", [(False, 32), (False, 64), (True, 32), (True, 64)])
def test_mobilenet_calibration_runs_and_is_reproducible(nat, residual, hw, monkeypatch, capsys):
    from common.quantity import merge_bn, _float_conv
    from model.mobilenet.MobileNet_fabu import MobileNet
    from tools import Quantity
    model = merge_bn(cases.seed_model(MobileNet(num_classes=10, input_size=hw, residual=residual), base_seed=3).eval()).cuda()
    batches = cases.calib_batches(3, (4, 3, hw, hw), seed=31)
    dws = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(dws) == 13
    tables = []
    for own in (True, True, False):
        with product_workdir(input_shape="1,3,%d,%d" % (hw, hw), device="gpu", max_cali_img_num=2) as tmp:
            q = Quantity(model)
            q.own_depthwise = own
            q.activation_quantize(batches)
            tables.append(open(tmp + "/test/workdir/feat.table", "rb").read())
            if own:
                assert q.timings["own_conv1x1_launches"] >= 13 * 3
                assert all(_float_conv.is_verified(m, "dw") and not _float_conv.is_off(m) for m in dws)
    assert tables[0] == tables[1] and len(tables[0]) > 0                             # two fresh Quantity objects: the same bytes
    rows_on, rows_off = tables[0].splitlines(), tables[2].splitlines()
    assert len(rows_on) == len(rows_off)
    with capsys.disabled():
        print("\n[depthwise f32] MobileNet residual=%s %dx%d: %d of %d feat.table rows differ between own_depthwise on and off"
              % (residual, hw, hw, sum(a != b for a, b in zip(rows_on, rows_off)), len(rows_on)))
    # per-channel calibration: the convolution alone (own_plain), statistics by its hooks
    calls, real = [], nat.dwconv_f32
    monkeypatch.setattr(nat, "dwconv_f32", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with product_workdir(input_shape="1,3,%d,%d" % (hw, hw), device="gpu", max_cali_img_num=2):
        q = Quantity(model)
        q.own_depthwise = True
        bits = q.activation_quantize_per_channel(batches)
    assert len(calls) >= 13 and len(bits) > 0


def test_mobilenet_at_224(nat):
    from common.quantity import merge_bn, _float_conv
    from model.mobilenet.MobileNet_fabu import MobileNet
    from tools import Quantity
    model = merge_bn(cases.seed_model(MobileNet(num_classes=10, input_size=224), base_seed=4).eval()).cuda()
    batches = cases.calib_batches(2, (8, 3, 224, 224), seed=41)
    dws = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    tables = []
    for _run in range(2):
        with product_workdir(input_shape="1,3,224,224", device="gpu", max_cali_img_num=1) as tmp:
            q = Quantity(model)
            q.own_depthwise = True
            q.activation_quantize(batches)
            tables.append(open(tmp + "/test/workdir/feat.table", "rb").read())
    assert tables[0] == tables[1] and len(tables[0]) > 0
    assert len(dws) == 13 and all(_float_conv.is_verified(m, "dw") and not _float_conv.is_off(m) for m in dws)
