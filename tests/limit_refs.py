"""Expected values for the size-limit tests (tests/test_gpu_size_limits.py), as a few fp32 torch operations each, so that they run on
the device in chunks of images: the oracle's plain loops take minutes at 10^9 outputs.  Test infrastructure, no product code.
tests/test_limit_refs_cpu.py holds every helper equal to the oracle, bit for bit, on small adversarial arrays.

Every helper takes and returns torch tensors on the operands' device and allocates a small multiple of its input: the callers hand
them chunks.  Powers of two are applied as fp32 multiplications: x * 2^-k is the correctly rounded image of the same real number
as the oracle's x / 2^k.
"""
import torch

I8_LO, I8_HI = -128.0, 127.0


def _pow2(k, like):
    """2^k as an fp32 scalar tensor on `like`'s device (|k| <= 120: normal); k may be an integer tensor (one power per channel)."""
    one = torch.ones((), dtype=torch.float32, device=like.device)
    return torch.ldexp(one, k if torch.is_tensor(k) else torch.tensor(int(k), device=like.device))


def quantity(x, ib):
    """Quantity.forward (oracle.quantity): clamp(rint(x * 2^ib), -128, 127), fp32."""
    return torch.round(x * _pow2(ib, x)).clamp(I8_LO, I8_HI)


def quandequan(x, bit):
    """QuanDequan.forward (oracle.quandequan): clamp(rint(x * 2^bit)) / 2^bit."""
    return quantity(x, bit) * _pow2(-bit, x)


def add_sat(a, b):
    """NewAdd.forward (oracle.add_sat): clamp(a + b, -128, 127)."""
    return (a + b).clamp(I8_LO, I8_HI)


def rightshift(x, rs):
    """RightShift.forward (oracle.rightshift): v = x / 2^rs, r = (int32) trunc(v + (v > 0 ? 0.5 : -0.5)) with a saturating cast,
    clamped to int8's range.  rs: an int, or an integer tensor that broadcasts against x (one shift per channel)."""
    v = x * _pow2(-rs if torch.is_tensor(rs) else -int(rs), x)
    w = v + torch.where(v > 0, 0.5, -0.5).to(torch.float32)
    return torch.trunc(w).clamp(-2147483648.0, 2147483520.0).clamp(I8_LO, I8_HI)


def recon_epilogue(acc, qbias, rs, ob):
    """The per-tensor tail (oracle.recon_epilogue) on acc [N][K][...]: RightShift(rs) -> + qbias[k] -> Sp -> DeQuantity(ob)."""
    shape = (1, -1) + (1,) * (acc.dim() - 2)
    return (rightshift(acc, rs) + qbias.view(shape)).clamp(I8_LO, I8_HI) * _pow2(-ob, acc)


def pc_epilogue(acc, qbias, rs_k, ob):
    """The per-channel tail (tests/per_channel_chain.pc_epilogue): channel k is shifted by rs_k[k] (an integer tensor [K])."""
    shape = (1, -1) + (1,) * (acc.dim() - 2)
    return (rightshift(acc, rs_k.view(shape)) + qbias.view(shape)).clamp(I8_LO, I8_HI) * _pow2(-ob, acc)


def relu(y):
    return torch.clamp_min(y, 0.0)


def add_resident(x, gx, y, gy, g_wide, ib, do_relu):
    """fq_add_resident's expression (include/fq.h; tests/int_conv_ref.add_resident_ref): integer tensors x, y standing for
    x * 2^-gx and y * 2^-gy -> (wide int16 = s * 2^g_wide, narrow int8 = clamp(rint(s * 2^ib))), s = clamp(x' + y', relu ? 0 : -128, 127).
    Every operand is a multiple of 2^-g_wide below 2^16 in magnitude: both terms, their sum and the scalings are exact in fp32."""
    assert g_wide == max(0, gx, gy) and g_wide <= 8
    s = x.to(torch.float32) * _pow2(-gx, x) + y.to(torch.float32) * _pow2(-gy, y)
    s = s.clamp(0.0 if do_relu else I8_LO, I8_HI)
    return (s * _pow2(g_wide, s)).to(torch.int16), quantity(s, ib).to(torch.int8)


def absmax(x, running=None):
    """DistributionCollector.refresh_max_val (oracle.absmax): max(|max x|, |min x|, running), an fp32 scalar tensor."""
    lo, hi = torch.aminmax(x.reshape(-1))
    m = torch.maximum(lo.abs(), hi.abs())
    return m if running is None else torch.maximum(m, running)


def hist2048(x, interval, hist=None, bins=2048):
    """_add_to_distribution (oracle.hist2048): for x != 0, hist[min((int32) fl32(|x| / interval), bins - 1)] += 1; quotients that
    are not below `bins` (inf and nan included) go to the last bin.  interval: a Python float that is an fp32 value, or an fp32
    scalar tensor.  Returns int64 [bins], added to `hist` when given.
    (On a GPU the quotient is only known to be correctly rounded when interval is a power of two: the GPU rows use such.)"""
    v = x.reshape(-1)
    v = v[v != 0].abs()
    iv = interval if torch.is_tensor(interval) else torch.tensor(interval, dtype=torch.float32, device=x.device)
    q = v / iv
    idx = torch.where(q < float(bins), q, torch.full_like(q, float(bins - 1))).to(torch.int64)
    h = torch.bincount(idx, minlength=bins)
    return h if hist is None else hist + h


def dequant_nhwc_to_nchw(q, g, channels):
    """fq_dequant_nhwc_to_nchw: integer NHWC [N][H][W][Cpad] -> fp32 NCHW [N][channels][H][W], value q * 2^-g."""
    return (q[..., :channels].to(torch.float32) * _pow2(-g, q)).permute(0, 3, 1, 2).contiguous()


def quantize_i8_nhwc(x, ib, cpad):
    """fq_quantize_i8_nhwc: fp32 NCHW -> int8 NHWC [N][H][W][cpad] = Quantity(x, ib), zeros in the padding channels."""
    n, c, h, w = x.shape
    out = torch.zeros((n, h, w, cpad), dtype=torch.int8, device=x.device)
    out[..., :c] = quantity(x, ib).to(torch.int8).permute(0, 2, 3, 1)
    return out


def maxpool_nhwc(q, kernel, stride, padding):
    """nn.MaxPool2d on an int8 NHWC tensor (max commutes with the de-quantisation): through torch's fp32 NCHW pooling."""
    y = torch.nn.functional.max_pool2d(q.permute(0, 3, 1, 2).to(torch.float32), kernel, stride, padding)
    return y.to(torch.int8).permute(0, 2, 3, 1).contiguous()


def avgpool_global_nhwc(q, g, channels):
    """fq_avgpool_global_nhwc: y[n][c] = (sum_hw q) * 2^-g / HW -- the integer sum (exact), one scaling, one fp32 division.
    (The divisor is a tensor on the operands' device: torch turns a division by a host scalar into a multiplication by its
    reciprocal on a GPU, which is not the correctly rounded quotient.)"""
    n, h, w, _ = q.shape
    s = q[..., :channels].to(torch.int32).sum(dim=(1, 2)).to(torch.float32)
    return (s * _pow2(-g, q)) / torch.tensor(float(h * w), dtype=torch.float32, device=q.device)


def conv1x1_f32(x, w, bias, stride=1):
    """A 1x1 convolution as ONE fp32 matmul per image chunk: w [Cout][Cin] @ x [n][Cin][HW].  Allowed only where the data make
    every partial sum an integer below 2^24 (the caller asserts sum_c |w| * max |x| + |b| < 2^24): the result is then exact in any
    order of summation."""
    if stride != 1:
        x = x[:, :, ::stride, ::stride]
    n, c, h, wd = x.shape
    y = torch.matmul(w, x.reshape(n, c, h * wd)) + bias.view(1, -1, 1)
    return y.view(n, -1, h, wd)


def conv_kxk_f32(x, w, bias, stride, pad):
    """An R x S convolution tap by tap: per tap one fp32 matmul over the shifted, zero-padded input.  The same integer bound as
    conv1x1_f32 (over all R * S * Cin terms)."""
    k, c, r, s = w.shape
    n, _, h, wd = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    y = bias.view(1, -1, 1).expand(n, k, ho * wo).clone()
    for a in range(r):
        for b in range(s):
            tap = xp[:, :, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride].reshape(n, c, ho * wo)
            y += torch.matmul(w[:, :, a, b], tap)
    return y.view(n, k, ho, wo)


def dwconv_taps(x, w, stride, pad):
    """A depthwise convolution tap by tap: x fp32 [n][C][H][W], w [C][1][R][S] -> sum over the taps of the shifted, zero-padded
    input times that tap's weight per channel.  No convolution library; exact where every partial sum is an integer below 2^24."""
    c, _, r, s = w.shape
    n, _, h, wd = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    y = torch.zeros((n, c, ho, wo), dtype=torch.float32, device=x.device)
    for a in range(r):
        for b in range(s):
            y += xp[:, :, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] * w[:, 0, a, b].view(1, c, 1, 1)
    return y


def gconv_taps(x, w, groups, stride, pad):
    """A grouped convolution tap by tap: x fp32 [n][C][H][W], w [K][C / groups][R][S]; per tap one batched fp32 matmul over the
    groups.  Exact where every partial sum is an integer below 2^24."""
    k, cgi, r, s = w.shape
    n, _, h, wd = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    y = torch.zeros((n, groups, k // groups, ho * wo), dtype=torch.float32, device=x.device)
    for a in range(r):
        for b in range(s):
            tap = xp[:, :, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride].reshape(n, groups, cgi, ho * wo)
            y += torch.matmul(w[:, :, a, b].reshape(groups, k // groups, cgi), tap)
    return y.view(n, k, ho, wo)


def first_mismatch(got, ref, base_elems, itemsize):
    """None when the two chunks are equal; else a sentence naming the first differing flat index of the WHOLE output (this chunk
    starts at element base_elems), its byte offset and how many multiples of 2^31 bytes lie before it."""
    if torch.equal(got, ref):
        return None
    if got.shape != ref.shape:
        return "shape %s, expected %s" % (tuple(got.shape), tuple(ref.shape))
    bad = (got != ref).reshape(-1)
    if got.dtype.is_floating_point:                         # (NaN != NaN: two NaNs at the same place are no mismatch)
        bad &= ~(torch.isnan(got) & torch.isnan(ref)).reshape(-1)
    if not bool(bad.any()):
        return None
    i = int(torch.nonzero(bad)[0])
    flat = base_elems + i
    return ("%d of %d elements of this chunk differ; first at flat index %d (byte offset %d, behind %d x 2^31 bytes): got %s, "
            "expected %s" % (int(bad.sum()), bad.numel(), flat, flat * itemsize, flat * itemsize >> 31,
                             got.reshape(-1)[i].item(), ref.reshape(-1)[i].item()))
