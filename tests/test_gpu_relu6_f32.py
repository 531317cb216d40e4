"""The `_act` entry points of the float convolutions (fq_conv1x1_f32_act, fq_conv1x1_sb_f32_act, fq_conv_kxk_f32_act,
fq_dwconv_f32_act): the clipped copy is torch's nn.ReLU6 of the kernel's own stored output bit for bit -- NaN,
+-inf, an exact 6 and its neighbours, an exact 0 and its neighbours included --, the y == NULL form writes the same copy, and the
stored output, the abs-max and the histogram are those of the call without an activation.  Operands are integer valued, so the
special values are exact.  (A -0 cannot leave these kernels: every output is an fma chain from +0 plus the bias, and +0 + -0 = +0.)
pytest -m gpu"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIX = np.float32(6)
# biases of the output channels whose weights are all zero: the output IS the bias there
SPECIAL = [SIX, np.float32(0), np.nextafter(SIX, np.float32(7)), np.nextafter(SIX, np.float32(0)), np.float32(1e-45),
           np.float32(-1e-45), np.float32(7), np.float32(-1)]


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _bits(t):
    return t.contiguous().view(torch.int32)


def _input(rng, shape):
    """Integer-valued activations in [-8, 8] with a NaN in the first channel and a +inf / a -inf in the last one (of the first and
    of the last image), at even coordinates, so that a stride-2 layer samples them too."""
    x = rng.integers(-8, 9, size=shape).astype(np.float32)
    x[0, 0, 0, 2], x[0, -1, 2, 2], x[-1, -1, 2, 2] = np.nan, np.inf, -np.inf
    return torch.from_numpy(x).cuda()


def _weights(rng, shape, special):
    """Integer-valued weights in [-3, 3]; the first `special` output channels are all zero (their output is their bias), the
    last one has no zero at all (0 * inf is NaN: its outputs under the two infinities stay infinite)."""
    w = rng.integers(-3, 4, size=shape).astype(np.float32)
    w[:special] = 0
    w[-1] = 2
    return w


def _bias(rng, cout, special, which):
    b = rng.integers(-4, 5, size=cout).astype(np.float32)
    b[:special] = np.resize(np.array(SPECIAL[4 * which:4 * which + 4] if special == 4 else SPECIAL, dtype=np.float32), special)
    return torch.from_numpy(b).cuda()


def _check(nat, call, shape_note, inf=True):
    """call(**epilogue) -> y runs one convolution; every property of the `_act` form against the form without.  (inf=False: the
    split-bf16 kernels turn a non-finite input into NaN, include/fq.h.)"""
    y0 = call()
    assert torch.isnan(y0).any() and (torch.isinf(y0).any() or not inf) and (y0 == 6).any() and (y0 == 0).any(), shape_note
    assert (y0 > 6).any() and ((y0 > 0) & (y0 < 6)).any() and (y0 < 0).any(), shape_note
    # the copy next to the stored output
    r = torch.empty_like(y0)
    y1 = call(relu_out=r, act=6.0)
    assert torch.equal(_bits(y1), _bits(y0)), shape_note                     # the stored output does not know about the activation
    want = torch.nn.functional.relu6(y1)
    assert torch.equal(_bits(r), _bits(want)), shape_note
    assert torch.isnan(r).any() and (r == 6).any() and (_bits(r) == 0).any()
    # ... and alone (y == NULL)
    r2 = torch.full_like(y0, -77.0)
    call(relu_out=r2, out=False, act=6.0)
    assert torch.equal(_bits(r2), _bits(r)), shape_note
    # nn.ReLU's copy is still nn.ReLU's
    r_plain = torch.empty_like(y0)
    call(relu_out=r_plain)
    assert torch.equal(_bits(r_plain), _bits(torch.nn.functional.relu(y0))) and not torch.equal(_bits(r_plain), _bits(r))
    # the statistics are the unclipped output's
    for out in (None, False):
        m0, m1 = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
        call(max_dev=m0, row=1, relu_out=torch.empty_like(y0), **({} if out is None else {"out": out}))
        ra = torch.empty_like(y0)
        call(max_dev=m1, row=1, relu_out=ra, act=6.0, **({} if out is None else {"out": out}))
        assert torch.equal(_bits(m0), _bits(m1)) and float(m1[0]) == 0.0 and torch.equal(_bits(ra), _bits(r)), shape_note
        assert float(m1[1]) > 6.0                                            # (finite: fmaxf drops NaN; inf is a value)
        iv = torch.tensor([0.5, 0.01], device="cuda")
        h0 = torch.zeros(2, 2048, dtype=torch.int64, device="cuda")
        h1 = torch.zeros(2, 2048, dtype=torch.int64, device="cuda")
        call(interval_dev=iv, hist_dev=h0, row=1, relu_out=torch.empty_like(y0), **({} if out is None else {"out": out}))
        rb = torch.empty_like(y0)
        call(interval_dev=iv, hist_dev=h1, row=1, relu_out=rb, act=6.0, **({} if out is None else {"out": out}))
        assert torch.equal(h0, h1) and int(h1[1].sum()) > 0 and int(h1[0].sum()) == 0 and torch.equal(_bits(rb), _bits(r)), shape_note
    # the contract's refusals
    with pytest.raises(nat.FqError):
        call(act=6.0)                                                        # no relu_out
    for cap in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(nat.FqError):
            call(relu_out=torch.empty_like(y0), act=cap)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("cin,cout,hw,n,stride,sb", [(16, 8, (5, 5), 2, 1, False), (20, 8, (5, 5), 2, 2, False), (32, 8, (5, 5), 2, 1, True)],
                         ids=["16to8", "20to8_k_tail_stride2", "32to8_split_bf16"])
def test_conv1x1_act(nat, cin, cout, hw, n, stride, sb, which):
    rng = np.random.default_rng(cin + which)
    x = _input(rng, (n, cin) + hw)
    w = torch.from_numpy(_weights(rng, (cout, cin), 6)).cuda()                  # six bias-only channels, two computed ones
    wt = nat.pack_sb_weight(w) if sb else w.t().contiguous()
    bias = _bias(rng, cout, 4, which)                                         # four of the special values per case ...
    bias[4], bias[5] = 6.0, 0.0                                               # ... and the exact 6 and 0 in both
    _check(nat, lambda **kw: nat.conv1x1_f32(x, wt, bias, stride, **kw), "c1 %d->%d" % (cin, cout), inf=not sb)


@pytest.mark.parametrize("cin", [16])
def test_conv_kxk_act(nat, cin):
    """3 x 3 stride 2 on 9 x 9, 16 -> 16 channels: the smallest input width fq_conv_kxk_f32 takes (Cin % 16 == 0; with 3 input
    channels both entry points answer FQ_ERR_UNSUPPORTED, and a 3-channel stem runs on the library convolution + the bias producer)."""
    rng = np.random.default_rng(9)
    x = _input(rng, (2, cin, 9, 9))
    w = torch.from_numpy(_weights(rng, (16, cin, 3, 3), 8)).cuda()
    bias = _bias(rng, 16, 8, 0)
    wt = nat.pack_kxk_weight(w)
    _check(nat, lambda **kw: nat.conv_kxk_f32(x, wt, bias, (3, 3), 2, 1, **kw), "kxk")
    x3 = _input(rng, (2, 3, 9, 9))
    w3 = nat.pack_kxk_weight(torch.zeros(16, 3, 3, 3, device="cuda"))
    for kw in ({}, {"relu_out": torch.empty(2, 16, 5, 5, device="cuda"), "act": 6.0}):
        with pytest.raises(nat.FqError, match="unsupported|UNSUPPORTED|not supported"):
            nat.conv_kxk_f32(x3, w3, bias, (3, 3), 2, 1, **kw)


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_act(nat, stride):
    rng = np.random.default_rng(19 + stride)
    x = _input(rng, (2, 19, 6, 11))
    w = torch.from_numpy(_weights(rng, (19, 1, 3, 3), 8)).cuda()
    bias = _bias(rng, 19, 8, 0)
    _check(nat, lambda **kw: nat.dwconv_f32(x, w, bias, (3, 3), stride, 1, **kw), "dw stride %d" % stride)
