"""fq_deconv_f32 -- the transposed float convolution of the calibration forward on the fp32 matrix cores, statistic in the epilogue
-- through the C ABI, through _float_conv with FQ_OWN_DECONV=1, and inside tools.Quantity (own_deconv).  Bit equality with the fmaf
chain of include/fq.h, exact agreement with a float64 reference on integer-valued data (every partial sum is exact, so an indexing or
tiling mistake shows as a wrong bit), the forms of the entry point bit for bit against each other, return codes, and calibrations of
a U-Net whose tables do not move.
    pytest -m gpu"""
import copy

import pytest
import torch
from torch import nn

from deconv_f32_util import BIG, CONTRACT_IDS, CONTRACT_SHAPES, IDS, SHAPES, emulate, macs, operands, out_hw, pack, ref64
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from common.quantity import _native
    _native.lib()
    return _native


def _run(nat, shape, x, wt, b, **kw):
    _N, _cin, _cout, _H, _W, R, S, stride, pad, outpad = shape
    return nat.deconv_f32(x, wt, b, (R, S), stride, pad, outpad, **kw)


_CASES = {}


def _case(shape, integer):
    """(x, w, wt, b, float64 reference, float64 bound, the kernel's plain output) of a shape, computed once and shared."""
    key = (shape, integer)
    if key not in _CASES:
        stride, pad, outpad = shape[7], shape[8], shape[9]
        x, w, b = operands(shape, integer)
        from common.quantity import _native
        xc, wc, bc = x.cuda(), pack(w).cuda(), b.cuda()
        _CASES[key] = (xc, w, wc, bc, ref64(x, w, b, stride, pad, outpad).cuda(),
                       ref64(x.abs(), w.abs(), b.abs(), stride, pad, outpad).cuda(), _run(_native, shape, xc, wc, bc))
    return _CASES[key]


@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=CONTRACT_IDS)
def test_the_stored_bits_are_the_fmaf_chain_of_the_header(nat, shape):
    """The numerics contract of include/fq.h: per output one fmaf chain over the taps of its phase, r then s ascending, c innermost,
    from +0.0f, a tap outside the image the operand +0.0f, then the bias -- evaluated on the host with libm's fmaf, on the
    Gaussian case."""
    x, w, wt, b, _ref, _bound, y = _case(shape, False)
    stride, pad, outpad = shape[7], shape[8], shape[9]
    want = emulate(x.cpu(), w, b.cpu(), stride, pad, outpad)
    got = y.cpu()
    assert got.shape == want.shape
    assert torch.equal(got, want), "%d of %d outputs differ, max %g" % (int((got != want).sum()), got.numel(),
                                                                       float((got - want).abs().max()))
    if macs(shape) < 20000:
        assert torch.equal(_run(nat, shape, x, wt, None).cpu(), emulate(x.cpu(), w, None, stride, pad, outpad))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_valued_data(nat, shape):
    x, w, wt, b, ref, bound, y = _case(shape, True)
    assert float(bound.max()) < 2 ** 24                                              # every partial sum is an exact integer
    assert y.shape == ref.shape and torch.equal(y.double(), ref)
    stride, pad, outpad = shape[7], shape[8], shape[9]
    assert torch.equal(_run(nat, shape, x, wt, None).double(), ref64(x, w, None, stride, pad, outpad).cuda())
    lib = torch.nn.functional.conv_transpose2d(x, w.cuda(), b, stride=stride, padding=pad, output_padding=outpad)
    assert torch.equal(y, lib)                                                       # F.conv_transpose2d's result exactly


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gaussian_data_within_the_bound_repeatable_and_independent_of_the_batch(nat, shape):
    from common.quantity import _float_conv
    x, w, wt, b, ref, bound, y = _case(shape, False)
    N, _cin, _cout, _H, _W, R, S, stride, pad, outpad = shape
    assert bool(((y.double() - ref).abs() <= _float_conv.TOL * bound).all())
    dref, dbound = _float_conv.dc_reference(x, w.cuda(), b, (R, S), (stride, stride), (pad, pad), (outpad, outpad))
    assert bool(((y - dref).abs() <= _float_conv.TOL * dbound).all())
    assert torch.equal(_run(nat, shape, x, wt, b), y)                                # same bits from run to run
    for i in range(N) if N > 1 else ():
        assert torch.equal(_run(nat, shape, x[i:i + 1].contiguous(), wt, b)[0], y[i]), i


def test_image_i_of_a_batch_of_three_has_the_bits_of_the_same_image_alone(nat):
    shape = (3, 32, 36, 5, 9, 3, 4, 2, 1, 1)
    x, w, b = operands(shape, False)
    x, wt, b = x.cuda(), pack(w).cuda(), b.cuda()
    y = _run(nat, shape, x, wt, b)
    for i in range(3):
        assert torch.equal(_run(nat, shape, x[i:i + 1].contiguous(), wt, b)[0], y[i]), i


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_forms_store_the_same_bits(nat, shape):
    x, _w, wt, b, _ref, _bound, y = _case(shape, False)
    amax = float(y.abs().max())
    # pass 1: the abs-max folded into an existing maximum, the ReLU copy
    mx = torch.tensor([0.0, 1e9, 0.0], device="cuda")
    r = torch.full_like(y, -7.0)
    y1 = _run(nat, shape, x, wt, b, max_dev=mx, row=2, relu_out=r)
    assert torch.equal(y1, y) and torch.equal(r, torch.relu(y))
    assert mx.tolist() == [0.0, 1e9, amax]
    _run(nat, shape, x, wt, b, max_dev=mx, row=1)
    assert float(mx[1]) == 1e9                                                       # a larger running maximum stays
    # pass 2: the histogram, accumulated onto existing counts, against the streaming kernel on the stored tensor; the last two
    # intervals lie outside the fast-quotient range (IEEE divide: everything in the last / first bin)
    for ivv in (amax / 2048 + 1e-12, 1e-30, 3e25):
        iv = torch.tensor([1.0, ivv], device="cuda")
        hist = torch.zeros(2, 2048, dtype=torch.int64, device="cuda")
        hist[1, 5] = 7
        want = hist.clone()
        y2 = _run(nat, shape, x, wt, b, interval_dev=iv, hist_dev=hist, row=1)
        nat.hist2048_seg([y], [1], iv, want)
        assert torch.equal(y2, y) and torch.equal(hist, want), ivv
        assert int(hist[1].sum()) - 7 == int((y != 0).sum()) and int(hist[0].sum()) == 0
    # only the ReLU's output wanted (y = NULL): the statistic is still that of y
    mx2 = torch.zeros(1, device="cuda")
    r2 = torch.full_like(y, -7.0)
    assert _run(nat, shape, x, wt, b, max_dev=mx2, row=0, relu_out=r2, out=False) is None
    assert torch.equal(r2, torch.relu(y)) and float(mx2[0]) == amax
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    iv = torch.tensor([amax / 2048 + 1e-12], device="cuda")
    r2.fill_(-7.0)
    _run(nat, shape, x, wt, b, interval_dev=iv, hist_dev=hist, row=0, relu_out=r2, out=False)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want) and torch.equal(r2, torch.relu(y))
    r3 = torch.full_like(y, -7.0)                                                    # the ReLU copy without a statistic
    assert torch.equal(_run(nat, shape, x, wt, b, relu_out=r3), y) and torch.equal(r3, torch.relu(y))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s is not BIG], ids=CONTRACT_IDS)
def test_a_view_at_an_odd_float_offset_is_stored_correctly(nat, shape):
    """y and relu_out between sentinel floats, at 4-byte (not 8- or 16-byte) aligned addresses: the narrower stores, and nothing
    outside the tensor."""
    x, _w, wt, b, _ref, _bound, y = _case(shape, False)
    for lead in (1, 3):
        buf = torch.full((y.numel() + 8,), 777.0, device="cuda")
        rbuf = torch.full((y.numel() + 8,), 777.0, device="cuda")
        view, rview = buf[lead:lead + y.numel()].view(y.shape), rbuf[lead:lead + y.numel()].view(y.shape)
        assert view.data_ptr() % 8 != 0
        _run(nat, shape, x, wt, b, out=view, relu_out=rview)
        assert torch.equal(view, y) and torch.equal(rview, torch.relu(y))
        for t in (buf, rbuf):
            assert bool((t[:lead] == 777.0).all()) and bool((t[lead + y.numel():] == 777.0).all())


def test_nan_infinity_and_zero_outputs(nat):
    """A NaN input reaches exactly the outputs float64 gives it; an Inf next to the border stays Inf (a tap outside the image is
    the operand 0, never a neighbouring row's or plane's value, which would make 0 * Inf = NaN of a finite output); a channel of zero
    weights and zero bias is exactly zero and is not counted by the histogram; the abs-max ignores NaN."""
    shape = (2, 16, 8, 5, 7, 3, 3, 2, 1, 1)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 16, 5, 7), generator=g).float().cuda()
    w = torch.randint(1, 5, (16, 8, 3, 3), generator=g).float()
    w[:, 5] = 0.0
    b = torch.zeros(8, device="cuda")
    x[1, 4, 2, 3] = float("nan")
    x[0, 0, 4, 6] = float("inf")                                                     # last pixel of a plane
    x[0, 1, 0, 0] = float("inf")                                                     # first pixel of the next
    ref = ref64(x, w, b, 2, 1, 1).cuda()
    mx = torch.zeros(1, device="cuda")
    r = torch.empty(2, 8, 10, 14, device="cuda")
    y = _run(nat, shape, x, pack(w).cuda(), b, max_dev=mx, row=0, relu_out=r)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isinf(y), torch.isinf(ref))
    assert torch.equal(torch.isnan(r), torch.isnan(ref))
    ok = torch.isfinite(y)
    assert bool(ok.any()) and torch.equal(y[ok].double(), ref[ok])
    assert float(mx[0]) == float("inf")                                              # Inf enters the maximum, NaN does not
    x[0, 0, 4, 6] = 1.0
    x[0, 1, 0, 0] = 1.0
    mx.zero_()
    y = _run(nat, shape, x, pack(w).cuda(), b, max_dev=mx, row=0)
    ok = ~torch.isnan(y)
    assert float(mx[0]) == float(y[ok].abs().max()) and int((~ok).sum()) > 0
    iv = torch.tensor([float(mx[0]) / 2048 + 1e-12], device="cuda")
    hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    want = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")
    _run(nat, shape, x, pack(w).cuda(), b, interval_dev=iv, hist_dev=hist, row=0)
    nat.hist2048_seg([y], [0], iv, want)
    assert torch.equal(hist, want) and int(hist.sum()) <= int((y != 0).sum())


def test_return_codes_and_nothing_is_launched(nat):
    L = nat.lib()
    x = torch.zeros(2, 32, 6, 6, device="cuda")
    w = torch.zeros(8 * 8 * 32 * 16, device="cuda")                                  # room for every geometry below
    b = torch.zeros(16, device="cuda")
    y = torch.full((2 * 16 * 40 * 40,), 4242.0, device="cuda")
    one = torch.zeros(2, device="cuda")
    h = torch.zeros(2048, dtype=torch.int64, device="cuda")
    X, Wp, B, Y = x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr()

    def call(xp=X, wp=Wp, bp=B, yp=Y, rp=None, N=2, Cin=16, H=6, W=6, Cout=8, R=3, S=3, stride=2, pad=1, outpad=1, mp=None, ip=None,
             hp=None):
        return L.fq_deconv_f32(xp, wp, bp, yp, rp, N, Cin, H, W, Cout, R, S, stride, pad, outpad, mp, ip, hp, None)

    # geometries the kernel declines: FQ_ERR_UNSUPPORTED, and fq_deconv_f32_supported says so too
    geoms = [(dict(Cin=24), False), (dict(Cout=6), False), (dict(R=9, S=9), False), (dict(stride=5), False), (dict(pad=3), False),
             (dict(outpad=2), False), (dict(R=3, S=2, pad=2), False)]
    for kw, ok in geoms:
        rc = call(**kw)
        assert rc == -4, (kw, rc)
        a = dict(Cin=16, Cout=8, R=3, S=3, stride=2, pad=1, outpad=1, H=6, W=6)
        a.update(kw)
        assert L.fq_deconv_f32_supported(a["Cin"], a["Cout"], 1, a["R"], a["S"], a["stride"], a["stride"], a["pad"], a["pad"], a["outpad"],
                                         a["outpad"], 1, 1, a["H"], a["W"]) == 0, kw
    assert L.fq_deconv_f32_supported(16, 8, 2, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 6, 6) == 0    # groups
    assert L.fq_deconv_f32_supported(16, 8, 1, 3, 3, 2, 2, 1, 1, 1, 1, 2, 2, 6, 6) == 0    # dilation
    assert L.fq_deconv_f32_supported(16, 8, 1, 3, 3, 1, 2, 1, 1, 0, 0, 1, 1, 6, 6) == 0    # stride 1 x 2
    assert L.fq_deconv_f32_supported(16, 8, 1, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 6, 6) == 1
    assert call(N=1 << 14, Cin=1 << 10, H=8, W=8) == -4                              # x of 2^30 elements
    assert call(N=1 << 16, Cout=1 << 10, H=2, W=2) == -4                             # y of 2^30 elements
    # invalid arguments: FQ_ERR_INVALID_ARG
    for kw in (dict(xp=None), dict(wp=None), dict(yp=None), dict(xp=X + 2), dict(wp=Wp + 4), dict(wp=Wp + 8), dict(yp=Y + 2),
               dict(bp=B + 2), dict(rp=Y + 1), dict(Cin=0), dict(H=0), dict(W=0), dict(Cout=0), dict(N=-1), dict(stride=0),
               dict(pad=-1), dict(outpad=-1), dict(R=0, S=0),
               dict(mp=one.data_ptr(), ip=one.data_ptr(), hp=h.data_ptr()), dict(hp=h.data_ptr()), dict(mp=one.data_ptr() + 2),
               dict(ip=one.data_ptr(), hp=h.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    assert call(N=0) == 0                                                            # an empty batch: FQ_OK
    torch.cuda.synchronize()
    assert bool((y == 4242.0).all())                                                 # nothing was launched
    with pytest.raises(nat.FqError):
        nat.deconv_f32(x[:, :24].contiguous(), torch.zeros(9 * 24, 8, device="cuda"), b[:8].contiguous(), (3, 3), 2, 1, 1)
    # ... and the calls that are taken write y, relu_out alone, or both
    assert call() == 0 and call(bp=None) == 0 and call(yp=None, rp=Y) == 0
    torch.cuda.synchronize()
    assert bool((y[:2 * 8 * 12 * 12] == 0.0).all()) and bool((y[2 * 8 * 12 * 12:] == 4242.0).all())


def test_float_conv_takes_transposed_layers_with_the_switch_on(nat, monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.setenv("FQ_OWN_DECONV", "1")
    up = nn.ConvTranspose2d(32, 24, 4, stride=2, padding=1).cuda().eval()
    x = torch.randn(3, 32, 6, 10, device="cuda")
    assert _float_conv.kind(up, x) == "dc" and _float_conv.kind(up, x, deconv=False) is None
    wt = _float_conv.weight(up, "dc")
    assert torch.equal(wt, pack(up.weight.detach())) and _float_conv.weight(up, "dc") is wt
    own = nat.deconv_f32(x, wt, up.bias.detach(), (4, 4), 2, 1, 0)
    with torch.no_grad():
        lib = up(x)
        assert own.shape == lib.shape and float((own - lib).abs().max()) <= 1e-4
        out = _float_conv.plain(up, "dc", x)
        assert torch.equal(out, own) and _float_conv.is_verified(up, "dc") and not _float_conv.is_off(up)
        calls, real = [], nat.deconv_f32
        monkeypatch.setattr(nat, "deconv_f32", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
        assert torch.equal(_float_conv.plain(up, "dc", x), own) and calls == [{}]      # checked once per process
        monkeypatch.setattr(nat, "deconv_f32", real)
        assert _float_conv.call_qd(up, x, 4, 8) is None                              # no QuanDequan form
        # a module that disagrees keeps the library's transposed convolution
        other = copy.deepcopy(up)
        monkeypatch.setattr(_float_conv, "TOL", -1.0)
        lib_out = _float_conv.plain(other, "dc", x)
        assert _float_conv.is_off(other) and not _float_conv.is_verified(other, "dc") and _float_conv.kind(other, x) is None
        assert lib_out.shape == own.shape and float((lib_out - own).abs().max()) <= 1e-4       # (the library's result)
        monkeypatch.setattr(_float_conv, "TOL", 1e-5)
        monkeypatch.setenv("FQ_OWN_DECONV", "0")
        assert _float_conv.kind(up, x) is None
    assert "forward" not in up.__dict__


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: model/unet/UNet_fabu.py with up="deconv" inside tools.Quantity

def _unet(up_kernel, integer, seed=11):
    """UNet(input_size 32, base_width 16, depth 2, up="deconv") behind merge_bn.  integer: small sparse integer parameters -- with
    integer images every partial sum of every layer is an integer below 2^24 (asserted by the caller), so every fp32 sum is exact
    whatever its order and whichever kernel computes it."""
    from common.quantity import merge_bn
    from model.unet.UNet_fabu import UNet
    torch.manual_seed(seed)
    model = UNet(num_classes=2, input_size=32, base_width=16, depth=2, batch_norm=True, up="deconv", up_kernel=up_kernel).eval()
    model = merge_bn(model)
    if integer:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in model.modules():
                if not isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                    continue
                # +-1 weights, about three per output (of fan-in products): thirteen layers deep the sums of absolute values
                # stay below 2^24 (about 2 * 10^6 here)
                p = m.weight
                fan = (p.shape[1] * p.shape[2] * p.shape[3] if isinstance(m, nn.Conv2d)
                       else p.shape[0] * -(-p.shape[2] // 2) * -(-p.shape[3] // 2))
                v = torch.randint(0, 2, p.shape, generator=g).float() * 2 - 1
                p.copy_(v * (torch.rand(p.shape, generator=g) < min(0.5, 3.0 / fan)).float())
                m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
    return model


def _peak(model, batches):
    """The largest partial sum any layer can reach: the float64 forward of |parameters| on |images|."""
    absnet = copy.deepcopy(model).double()
    with torch.no_grad():
        for p in absnet.parameters():
            p.abs_()
    peak, hooks = [0.0], []
    for m in absnet.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            hooks.append(m.register_forward_hook(lambda mod, i, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))))
    with torch.no_grad():
        for images, _ in batches:
            absnet(images.double().abs())
    return peak[0]


def _calibrate(model, batches, own, monkeypatch):
    """One calibration on the GPU: (bits, feat.table bytes, abs-max values, histograms, timings, calls of torch's
    nn.ConvTranspose2d.forward per batch position, the model on the device)."""
    from tools import Quantity
    entered = []
    real = nn.ConvTranspose2d.forward

    def counted(self, x, output_size=None):
        entered.append(1)
        return real(self, x, output_size)

    monkeypatch.setattr(nn.ConvTranspose2d, "forward", counted)
    try:
        with product_workdir(input_shape="1,3,32,32", device="gpu", max_cali_img_num=3) as tmp:
            net = copy.deepcopy(model).cuda()
            q = Quantity(net)
            del entered[:]                                                            # (the constructor's trace forward)
            q.own_deconv = own
            bits = q.activation_quantize(list(batches))
            table = open(tmp + "/test/workdir/feat.table", "rb").read()
            return (dict(bits), table, dict(q._collector.max_vals), q._collector.hist_device.clone(), dict(q.timings), len(entered),
                    net)
    finally:
        monkeypatch.setattr(nn.ConvTranspose2d, "forward", real)


@pytest.mark.parametrize("up_kernel", (2, 3, 4))
def test_unet_calibration_with_the_kernel_is_byte_identical_on_exact_data(up_kernel, monkeypatch):
    from common.quantity import _float_conv
    g = torch.Generator().manual_seed(21 + up_kernel)
    batches = [(torch.randint(-2, 3, (4, 3, 32, 32), generator=g).float(), torch.zeros(4, dtype=torch.long)) for _ in range(5)]
    model = _unet(up_kernel, True)
    peak = _peak(model, batches)
    assert 0 < peak < 2 ** 24, peak
    off = _calibrate(model, batches, False, monkeypatch)
    off2 = _calibrate(model, batches, False, monkeypatch)
    on = _calibrate(model, batches, True, monkeypatch)
    assert on[0] == off[0] and on[1] == off[1] and len(on[1]) > 0 and on[2] == off[2] and torch.equal(on[3], off[3])
    assert int(on[3].sum()) > 0
    ups = list(on[6].ups)
    assert len(ups) == 2 and all(_float_conv.is_verified(m, "dc") and not _float_conv.is_off(m) for m in ups)
    assert not any(_float_conv.is_verified(m) for m in off[6].ups)
    # both up-convolutions are counted: two launches per pass-1 batch (batches 0 .. MAX_CALI_IMG_NUM)
    assert on[4]["own_conv1x1_launches"] - off[4]["own_conv1x1_launches"] == 2 * 4, (on[4], off[4])
    # torch's nn.ConvTranspose2d.forward is never entered with the switch on (the once-per-process check is library-free too) ...
    assert on[5] == 0, on[5]
    # ... and with the switch off the calibration is what the parent commit gives for this model and input (measured there with
    # these helpers): torch's forward entered 2 up-convolutions x 5 batches x 2 passes = 20 times (nothing is cached: pass 2
    # runs every forward again), 36 own launches (9 of the 11 nn.Conv2d x the 4 pass-1 batches), 44 fused histogram launches
    assert off[5] == off2[5] == 20, off[5]
    assert off[4]["own_conv1x1_launches"] == 36 and on[4]["own_conv1x1_launches"] == 36 + 2 * 4
    assert off[4]["fused_hist_launches"] == 44 and off[4]["fused_bias_absmax_convs"] == 11 and off[4]["fused_relus"] == 10
    strip = lambda t: {k: v for k, v in t.items() if not k.endswith("_s")}            # noqa: E731  (wall times differ)
    assert strip(off[4]) == strip(off2[4]) and off[1] == off2[1]


def test_unet_tables_on_gaussian_weights_are_the_same(monkeypatch, capsys):
    """Random parameters: the kernel's sums differ from the library's in their last bits (another summation order), which could move
    a value across a bin edge; on this model and input no row of the table moves (DESIGN.md section 36 records the count: 0 of 16 for
    every up_kernel), so the comparison is an assertion."""
    batches = [(torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(40 + i)), torch.zeros(4, dtype=torch.long))
               for i in range(5)]
    for up_kernel in (2, 3, 4):
        model = _unet(up_kernel, False)
        off = _calibrate(model, batches, False, monkeypatch)
        on = _calibrate(model, batches, True, monkeypatch)
        on2 = _calibrate(model, batches, True, monkeypatch)
        assert on[1] == on2[1] and len(on[1]) > 0                                    # two fresh Quantity objects: the same bytes
        rows_on, rows_off = on[1].splitlines(), off[1].splitlines()
        assert len(rows_on) == len(rows_off) and on[5] == 0
        with capsys.disabled():
            print("\n[deconv f32] UNet(32, 16, depth 2) up_kernel %d, Gaussian weights: %d of %d feat.table rows differ between "
                  "own_deconv on and off" % (up_kernel, sum(u != v for u, v in zip(rows_on, rows_off)), len(rows_on)))
        assert rows_on == rows_off
