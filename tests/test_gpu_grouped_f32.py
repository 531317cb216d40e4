"""fq_gconv_f32 -- the grouped float convolution of the calibration forward, statistic in the epilogue -- through the C ABI,
through _float_conv with FQ_OWN_GCONV=1, and inside tools.Quantity (own_grouped).  Exact agreement with a float64 reference on
integer-valued data (every partial sum is exact, so an indexing or tiling mistake shows as a wrong bit), the project's
summation-order bound on Gaussian data, bit equality with the fmaf chain of include/fq.h, the forms of the entry point bit for bit
against each other, padding and group boundaries that leak nothing, return codes, and calibrations whose tables do not move.
    pytest -m gpu"""
import copy

import pytest
import torch
from torch import nn

import cases
import grouped_nets
from grouped_f32_util import CONTRACT_SHAPES, IDS, SHAPES, emulate, macs, operands, ref64
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from common.quantity import _native
    _native.lib()
    return _native


def _run(nat, shape, x, w, b, **kw):
    _N, G, _cgi, _cgo, _H, _W, R, stride, pad = shape
    return nat.gconv_f32(x, w, b, G, (R, R), stride, pad, **kw)


_CASES = {}


def _case(shape, integer):
    """(x, w, b, float64 reference, float64 bound, the kernel's plain output) of a shape, computed once and shared."""
    key = (shape, integer)
    if key not in _CASES:
        G, stride, pad = shape[1], shape[7], shape[8]
        x, w, b = operands(shape, integer)
        from common.quantity import _native
        xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
        _CASES[key] = (xc, wc, bc, ref64(x, w, b, G, stride, pad).cuda(), ref64(x.abs(), w.abs(), b.abs(), G, stride, pad).cuda(),
                       _run(_native, shape, xc, wc, bc))
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_valued_data(nat, shape):
    x, w, b, ref, bound, y = _case(shape, True)
    assert float(bound.max()) < 2 ** 24                                              # every partial sum is an exact integer
    assert y.shape == ref.shape and torch.equal(y.double(), ref)
    G, stride, pad = shape[1], shape[7], shape[8]
    assert torch.equal(_run(nat, shape, x, w, None).double(), ref64(x, w, None, G, stride, pad).cuda())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gaussian_data_within_the_bound_repeatable_and_independent_of_the_batch(nat, shape):
    from common.quantity import _float_conv
    x, w, b, ref, bound, y = _case(shape, False)
    N, G, cgi, cgo, H, W, R, stride, pad = shape
    assert bool(((y.double() - ref).abs() <= _float_conv.TOL * bound).all())
    gref, gbound = _float_conv.g_reference(x, w, b, G, (R, R), (stride, stride), (pad, pad))
    assert bool(((y.view(N, G * cgo, -1) - gref).abs() <= _float_conv.TOL * gbound).all())
    assert torch.equal(_run(nat, shape, x, w, b), y)                                 # same bits from run to run
    for i in sorted({0, N // 2, N - 1}) if N > 1 else ():
        assert torch.equal(_run(nat, shape, x[i:i + 1].contiguous(), w, b)[0], y[i]), i


@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=["x".join(map(str, s)) for s in CONTRACT_SHAPES])
def test_the_stored_bits_are_the_fmaf_chain_of_the_header(nat, shape):
    """The numerics contract of include/fq.h: per output one fmaf chain over (r, s, c), c innermost, from +0.0f, then the bias --
    evaluated on the host with libm's fmaf, on the Gaussian case.  The shapes cover every <R, stride> instantiation, a chunked
    group, several column blocks and several row bands (tests/test_grouped_f32_cpu.py asserts that)."""
    x, w, b, _ref, _bound, y = _case(shape, False)
    G, stride, pad = shape[1], shape[7], shape[8]
    want = emulate(x.cpu(), w.cpu(), b.cpu(), G, stride, pad)
    got = y.cpu()
    assert torch.equal(got, want), "%d of %d outputs differ, max %g" % (int((got != want).sum()), got.numel(),
                                                                       float((got - want).abs().max()))
    if macs(shape) < 20000:
        assert torch.equal(_run(nat, shape, x, w, None).cpu(), emulate(x.cpu(), w.cpu(), None, G, stride, pad))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_forms_store_the_same_bits(nat, shape):
    x, w, b, _ref, _bound, y = _case(shape, False)
    amax = float(y.abs().max())
    # pass 1: the abs-max folded into an existing maximum, the ReLU copy
    mx = torch.tensor([0.0, 1e9, 0.0], device="cuda")
    r = torch.full_like(y, -7.0)
    y1 = _run(nat, shape, x, w, b, max_dev=mx, row=2, relu_out=r)
    assert torch.equal(y1, y) and torch.equal(r, torch.clamp_min(y, 0))
    assert mx.tolist() == [0.0, 1e9, amax]
    _run(nat, shape, x, w, b, max_dev=mx, row=1)
    assert float(mx[1]) == 1e9                                                       # a larger running maximum stays
    # pass 2: the histogram, accumulated onto existing counts, against the streaming kernel on the plain output; the last two
    # intervals lie outside the fast-quotient range (IEEE divide: everything in the last / first bin)
    for ivv in (amax / 2048 + 1e-12, 1e-30, 3e25):
        iv = torch.tensor([1.0, ivv], device="cuda")
        hist = torch.zeros(2, 2048, dtype=torch.int64, device="cuda")
        hist[1, 5] = 7
        want = hist.clone()
        y2 = _run(nat, shape, x, w, b, interval_dev=iv, hist_dev=hist, row=1)
        nat.hist2048_seg([y], [1], iv, want)
        assert torch.equal(y2, y) and torch.equal(hist, want), ivv
        assert int(hist[1].sum()) - 7 == int((y != 0).sum()) and int(hist[0].sum()) == 0
    # only the ReLU's output wanted: y's allocation is not touched, the statistic is still that of y
    sentinel = torch.full_like(y, 12345.0)
    mx2 = torch.zeros(1, device="cuda")
    r2 = torch.full_like(y, -7.0)
    assert _run(nat, shape, x, w, b, max_dev=mx2, row=0, relu_out=r2, out=False) is None
    assert torch.equal(r2, torch.clamp_min(y, 0)) and float(mx2[0]) == amax and bool((sentinel == 12345.0).all())
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    iv = torch.tensor([amax / 2048 + 1e-12], device="cuda")
    r2.fill_(-7.0)
    _run(nat, shape, x, w, b, interval_dev=iv, hist_dev=hist, row=0, relu_out=r2, out=False)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want) and torch.equal(r2, torch.clamp_min(y, 0)) and bool((sentinel == 12345.0).all())
    # TestConv's form: QuanDequan of the plain output
    for bit, bw in ((4, 8), (-1, 8), (9, 16)):
        assert torch.equal(_run(nat, shape, x, w, b, qd=(bit, bw)), nat.quandequan(y, bit, bw)), (bit, bw)


def test_nan_and_zero_outputs(nat):
    shape = (2, 3, 4, 4, 9, 11, 3, 1, 1)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 12, 9, 11), generator=g).float().cuda()
    w = torch.randint(-4, 5, (12, 4, 3, 3), generator=g).float().cuda()
    w[w == 0] = 1.0                                                                  # (every window that covers a NaN is NaN either way: 0 * NaN)
    w[5] = 0.0                                                                       # exactly-zero outputs: a whole channel
    b = torch.zeros(12, device="cuda")
    x[1, 4, 3, 5] = float("nan")                                                     # group 1: NaN in its 4 output channels, 9 outputs each
    x[0, 0, 8, 10] = float("nan")                                                    # a corner: its window is cut by the padding
    ref = ref64(x, w, b, 3, 1, 1).cuda()
    mx = torch.zeros(1, device="cuda")
    r = torch.empty(2, 12, 9, 11, device="cuda")
    y = _run(nat, shape, x, w, b, max_dev=mx, row=0, relu_out=r)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and int(torch.isnan(y).sum()) == 4 * (9 + 4)
    assert torch.equal(torch.isnan(r), torch.isnan(ref))
    ok = ~torch.isnan(y)
    assert torch.equal(y[ok].double(), ref[ok]) and bool((y[0, 5] == 0).all()) and bool((y[1, 5][ok[1, 5]] == 0).all())
    assert float(mx[0]) == float(y[ok].abs().max())                                 # NaN does not enter the maximum
    iv = torch.tensor([float(mx[0]) / 2048 + 1e-12], device="cuda")
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    _run(nat, shape, x, w, b, interval_dev=iv, hist_dev=hist, row=0)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want)
    assert int(hist.sum()) <= int((y != 0).sum())                                    # exact zeros are not counted


@pytest.mark.parametrize("R,stride,pad", [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (1, 1, 0), (1, 2, 0)])
def test_no_value_leaks_across_groups_planes_or_the_padding(nat, R, stride, pad):
    """+Inf in the first channel of the NEXT group (at every pixel of one plane), and at the last element of plane p and the first
    element of plane p + 1: a group's outputs must stay what float64 has -- finite where no tap of the group touches an Inf.
    The padded taps next to the Infs must be the operand 0, never the neighbouring plane's (or row's) element: an Inf that leaked
    would make a finite output non-finite, and 0 * Inf a NaN.  The output is a view between sentinel floats, at an odd float
    offset."""
    from common.quantity import _float_conv
    N, G, cgi, cgo, H, W = 2, 3, 4, 8, 9, 7
    shape = (N, G, cgi, cgo, H, W, R, stride, pad)
    g = torch.Generator().manual_seed(R * 10 + stride + pad)
    x = torch.randn(N, G * cgi, H, W, generator=g).cuda()
    w = (torch.randn(G * cgo, cgi, R, R, generator=g).abs() + 0.1).cuda()
    b = torch.randn(G * cgo, generator=g).cuda()
    x[0, 2 * cgi] = float("inf")                                                     # image 0: the channel behind group 1's last
    planes = x.view(N * G * cgi, H, W)
    for p in (1, 11, 14):                                                            # plane 11 -> 12 crosses the image boundary
        planes[p, H - 1, W - 1] = float("inf")
        planes[p + 1, 0, 0] = float("inf")
    ref = ref64(x, w, b, G, stride, pad).cuda()
    finite = torch.isfinite(ref)
    assert bool(finite.any()) and not bool(finite.all())
    assert bool(finite[0, cgo:2 * cgo].any()) and not bool(finite[0, 2 * cgo:].any())    # group 1 of image 0 next to a group of Infs
    xf = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    bound = ref64(xf.abs(), w.abs(), b.abs(), G, stride, pad).cuda()
    buf = torch.full((ref.numel() + 8,), 777.0, device="cuda")
    y = buf[3:3 + ref.numel()].view(ref.shape)
    assert y.data_ptr() % 16 != 0
    _run(nat, shape, x, w, b, out=y)
    assert bool((buf[:3] == 777.0).all()) and bool((buf[3 + ref.numel():] == 777.0).all())
    assert torch.equal(torch.isfinite(y), finite) and torch.equal(torch.isnan(y), torch.isnan(ref))
    assert bool(((y.double() - ref).abs()[finite] <= _float_conv.TOL * bound[finite]).all())


def test_return_codes(nat):
    L = nat.lib()
    x = torch.zeros(2, 16, 6, 6, device="cuda")
    w = torch.zeros(64, 16, 3, 3, device="cuda")                                    # room for every geometry below
    b = torch.zeros(64, device="cuda")
    y = torch.zeros(2, 64, 16, 16, device="cuda")
    one = torch.zeros(2, device="cuda")
    h = torch.zeros(2048, dtype=torch.int64, device="cuda")
    X, Wp, B, Y = x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr()

    def call(xp=X, wp=Wp, bp=B, yp=Y, rp=None, N=2, C=16, H=6, W=6, K=16, G=2, R=3, S=3, stride=1, pad=1, mp=None, ip=None, hp=None):
        return L.fq_gconv_f32(xp, wp, bp, yp, rp, N, C, H, W, K, G, R, S, stride, pad, mp, ip, hp, None)

    assert call() == 0 and call(bp=None) == 0 and call(yp=None, rp=Y) == 0
    # geometries the kernel declines: FQ_ERR_UNSUPPORTED, and fq_gconv_f32_supported says so too
    geoms = [(dict(), True), (dict(R=1, S=1, pad=0), True), (dict(stride=2, pad=0), True), (dict(H=1, W=1), True),
             (dict(K=32, G=4), True), (dict(pad=2), True), (dict(R=1, S=1, pad=0, stride=2), True),
             (dict(G=16), False), (dict(G=1), False), (dict(G=8), False), (dict(C=12, K=12), False), (dict(G=3), False),
             (dict(K=24, G=4), False), (dict(R=5, S=5, pad=2), False), (dict(R=3, S=1), False), (dict(stride=3), False),
             (dict(pad=3), False), (dict(R=1, S=1, pad=1), False), (dict(H=2, pad=0), False), (dict(W=1, pad=0), False)]
    for kw, ok in geoms:
        rc = call(**kw)
        assert rc == (0 if ok else -4), (kw, rc)
        a = dict(C=16, K=16, G=2, R=3, S=3, stride=1, pad=1, H=6, W=6)
        a.update({k: v for k, v in kw.items() if k in a})
        assert L.fq_gconv_f32_supported(a["C"], a["K"], a["G"], a["R"], a["S"], a["stride"], a["stride"], a["pad"], a["pad"], 1, 1,
                                        a["H"], a["W"]) == int(ok), kw
    assert L.fq_gconv_f32_supported(16, 16, 2, 3, 3, 1, 1, 1, 1, 2, 2, 6, 6) == 0    # dilation
    assert L.fq_gconv_f32_supported(16, 16, 2, 3, 3, 1, 2, 1, 1, 1, 1, 6, 6) == 0    # stride (1, 2)
    assert L.fq_gconv_f32_supported(16, 16, 2, 3, 3, 1, 1, 1, 2, 1, 1, 6, 6) == 0    # padding (1, 2)
    assert L.fq_gconv_f32_supported(136, 136, 2, 3, 3, 1, 1, 1, 1, 1, 1, 6, 6) == 0  # 68 per group
    assert L.fq_gconv_f32_supported(0, 16, 2, 3, 3, 1, 1, 1, 1, 1, 1, 6, 6) == 0
    assert call(N=1 << 14, C=1 << 10, K=1 << 10, G=1 << 8, H=8, W=8) == -4           # 2^30 elements
    # invalid arguments: FQ_ERR_INVALID_ARG
    for kw in (dict(xp=None), dict(wp=None), dict(yp=None), dict(xp=X + 2), dict(wp=Wp + 1), dict(yp=Y + 2), dict(bp=B + 2),
               dict(rp=Y + 1), dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(K=0), dict(G=0), dict(N=-1), dict(stride=0),
               dict(pad=-1), dict(R=0, S=0),
               dict(mp=one.data_ptr(), ip=one.data_ptr(), hp=h.data_ptr()), dict(hp=h.data_ptr()), dict(mp=one.data_ptr() + 2),
               dict(ip=one.data_ptr(), hp=h.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    qd = lambda bit, bw, yp=Y: L.fq_gconv_qd_f32(X, Wp, B, yp, 2, 16, 6, 6, 16, 2, 3, 3, 1, 1, bit, bw, None)
    assert qd(4, 8) == 0 and qd(4, 7) == -1 and qd(121, 8) == -1 and qd(4, 8, None) == -1
    assert L.fq_gconv_qd_f32(X, Wp, B, Y, 2, 16, 6, 6, 16, 2, 5, 5, 1, 2, 4, 8, None) == -4
    torch.cuda.synchronize()
    with pytest.raises(nat.FqError):
        nat.gconv_f32(x, torch.zeros(16, 8, 5, 5, device="cuda"), b[:16].contiguous(), 2, (5, 5), 1, 2)


def test_float_conv_takes_grouped_layers_with_the_switch_on(nat, monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.setenv("FQ_OWN_GCONV", "1")
    monkeypatch.delenv("FQ_OWN_DWCONV", raising=False)
    conv = nn.Conv2d(24, 48, 3, stride=2, padding=1, groups=3).cuda().eval()
    x = torch.randn(3, 24, 14, 14, device="cuda")
    assert _float_conv.kind(conv, x) == "g" and _float_conv.kind(conv, x, grouped=False) is None
    assert _float_conv.weight(conv, "g").data_ptr() == conv.weight.data_ptr()
    own = nat.gconv_f32(x, conv.weight.detach(), conv.bias.detach(), 3, (3, 3), 2, 1)
    seen = []
    handle = conv.register_forward_hook(lambda m, i, o: seen.append(o))
    with torch.no_grad():
        out = _float_conv.call(conv, x)
        assert len(seen) == 1 and seen[0] is out and torch.equal(out, own)           # the kernel's tensor; hooks fire
        assert _float_conv.is_verified(conv, "g") and not _float_conv.is_off(conv) and "forward" not in conv.__dict__
        calls, real = [], nat.gconv_f32
        monkeypatch.setattr(nat, "gconv_f32", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
        _float_conv.call(conv, x)
        assert calls == [{}]                                                         # checked once per process: the plain run alone
        del calls[:]
        assert _float_conv.call_qd(conv, x, 4, 8) is None and not calls               # somebody watches the un-quantised output
        handle.remove()
        fused = _float_conv.call_qd(conv, x, 4, 8)
        assert len(calls) == 1 and calls[0] == {"qd": (4, 8)} and torch.equal(fused, nat.quandequan(own, 4))
        monkeypatch.setattr(nat, "gconv_f32", real)
        # the trace forward of Quantity's constructor takes the layer too
        with _float_conv.own_convs(conv):
            assert torch.equal(conv(x), own)
        # a module that disagrees keeps the library convolution
        other = copy.deepcopy(conv)
        monkeypatch.setattr(_float_conv, "TOL", -1.0)
        lib_out = _float_conv.call(other, x)
        assert _float_conv.is_off(other) and not _float_conv.is_verified(other, "g") and _float_conv.kind(other, x) is None
        assert torch.equal(lib_out, nn.Conv2d.forward(other, x))
        monkeypatch.setattr(_float_conv, "TOL", 1e-5)
        assert float((lib_out - own).abs().max()) <= 1e-4
        # declined layers stay None with the switch on (a depthwise one waits for its own switch); with it off so does this one
        assert _float_conv.kind(nn.Conv2d(16, 16, 3, padding=1, groups=8).cuda(), torch.zeros(1, 16, 8, 8, device="cuda")) is None
        dw = nn.Conv2d(16, 16, 3, padding=1, groups=16).cuda()
        assert _float_conv.kind(dw, torch.zeros(1, 16, 8, 8, device="cuda")) is None
        assert _float_conv.kind(dw, torch.zeros(1, 16, 8, 8, device="cuda"), depthwise=True) == "dw"
        monkeypatch.setenv("FQ_OWN_GCONV", "0")
        assert _float_conv.kind(conv, x) is None


def _integer_resnext():
    """grouped_nets.ToyResNeXt with small sparse integer parameters: every partial sum of every convolution is an integer below
    2^24 (asserted by the caller), so every fp32 sum is exact whatever its order."""
    model = grouped_nets.ToyResNeXt().eval()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 4:
                keep = 0.5 if p.shape[1] <= 4 else 0.125
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
    batches = [(torch.randint(-2, 3, (4, 3, 8, 8), generator=g).float(), torch.zeros(4, dtype=torch.long)) for _ in range(5)]
    # the bound, on the host in float64: the forward of |parameters| on |images| dominates every partial sum of every layer
    absnet = copy.deepcopy(_integer_resnext()).double()
    with torch.no_grad():
        for p in absnet.parameters():
            p.abs_()
    peak, hooks = [0.0], []
    for m in absnet.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)) or type(m).__name__ == "Eltwise":
            hooks.append(m.register_forward_hook(lambda mod, i, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))))
    with torch.no_grad():
        for images, _ in batches:
            absnet(images.double().abs())
    assert 0 < peak[0] < 2 ** 24, peak
    runs = []
    for own in (True, False):
        with product_workdir(input_shape="1,3,8,8", device="gpu", max_cali_img_num=3) as tmp:
            q = Quantity(_integer_resnext().cuda())
            q.own_grouped = own
            bits = q.activation_quantize(batches)
            runs.append((dict(bits), open(tmp + "/test/workdir/feat.table", "rb").read(), dict(q._collector.max_vals),
                         q._collector.hist_device.clone(), q.timings["own_conv1x1_launches"]))
            gs = [q.model.b1.conv2, q.model.b2.conv2]
            if own:
                assert all(_float_conv.is_verified(m, "g") and not _float_conv.is_off(m) for m in gs)
            else:
                assert not any(_float_conv.is_verified(m) for m in gs)
    on, off = runs
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and torch.equal(on[3], off[3])
    assert int(on[3].sum()) > 0
    assert on[4] - off[4] == 2 * 4, (on[4], off[4])         # two grouped layers x pass-1 batches (batches 0 .. MAX_CALI_IMG_NUM)


def _resnext50(hw, seed):
    from common.quantity import merge_bn
    from model.resnext.ResNeXt_fabu import ResNeXt50
    model = merge_bn(cases.seed_model(ResNeXt50(num_classes=10, input_size=hw), base_seed=seed).eval()).cuda()
    gs = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(gs) == 16
    return model, gs


@pytest.mark.parametrize("hw", [32, 64])
def test_resnext50_calibration_runs_and_is_reproducible(nat, hw, monkeypatch, capsys):
    from common.quantity import _float_conv
    from tools import Quantity
    model, gs = _resnext50(hw, 3)
    batches = cases.calib_batches(2, (4, 3, hw, hw), seed=31)                        # 8 images
    tables = []
    for own in (True, True, False):
        with product_workdir(input_shape="1,3,%d,%d" % (hw, hw), device="gpu", max_cali_img_num=1) as tmp:
            q = Quantity(model)
            q.own_grouped = own
            q.activation_quantize(batches)
            tables.append(open(tmp + "/test/workdir/feat.table", "rb").read())
            if own:
                assert q.timings["own_conv1x1_launches"] >= 16 * 2
                assert all(_float_conv.is_verified(m, "g") and not _float_conv.is_off(m) for m in gs)
    assert tables[0] == tables[1] and len(tables[0]) > 0                             # two fresh Quantity objects: the same bytes
    rows_on, rows_off = tables[0].splitlines(), tables[2].splitlines()
    assert len(rows_on) == len(rows_off)
    with capsys.disabled():
        print("\n[grouped f32] ResNeXt50 %dx%d: %d of %d feat.table rows differ between own_grouped on and off"
              % (hw, hw, sum(a != b for a, b in zip(rows_on, rows_off)), len(rows_on)))
    # per-channel calibration: the convolution alone (own_plain), statistics by its hooks
    calls, real = [], nat.gconv_f32
    monkeypatch.setattr(nat, "gconv_f32", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with product_workdir(input_shape="1,3,%d,%d" % (hw, hw), device="gpu", max_cali_img_num=1):
        q = Quantity(model)
        q.own_grouped = True
        bits = q.activation_quantize_per_channel(batches)
    assert len(calls) >= 16 and len(bits) > 0


def test_resnext50_at_224(nat):
    from common.quantity import _float_conv
    from tools import Quantity
    model, gs = _resnext50(224, 4)
    batches = cases.calib_batches(2, (4, 3, 224, 224), seed=41)                      # 8 images
    with product_workdir(input_shape="1,3,224,224", device="gpu", max_cali_img_num=1) as tmp:
        q = Quantity(model)
        q.own_grouped = True
        q.activation_quantize(batches)
        table = open(tmp + "/test/workdir/feat.table", "rb").read()
    assert len(table) > 0 and q.timings["own_conv1x1_launches"] >= 16 * 2
    assert all(_float_conv.is_verified(m, "g") and not _float_conv.is_off(m) for m in gs)
