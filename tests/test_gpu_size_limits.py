"""Every kernel just under its size limit (or, where it indexes with 64 bits and has none, beyond 2^31 bytes), against references
computed on the device in chunks (tests/limit_refs.py, tied to the CPU oracle by tests/test_limit_refs_cpu.py).

An overflow at these sizes is silent: a raw-buffer descriptor drops what lies past its records, a wrapped offset lands inside the
tensor and overwrites the first images.  So every element of every output is compared (torch.equal per chunk; a mismatch names the
first differing index and how many multiples of 2^31 bytes lie before it), the data are integer valued (equality is exact in any
order of summation) and come from a hash of the flat index (no two images, and no two positions 2^32 bytes apart, are equal).
The rows and the bytes each allocates are tests/size_limit_cases.GPU_CASES; a row whose declared peak does not fit the free
memory is skipped with that reason.  The refused side of every guard: tests/test_size_guards_cpu.py.      pytest -m gpu"""
import gc
import time

import pytest
import torch

import limit_refs as lr
import size_limit_cases as T

CASES = {c.id: c for c in T.GPU_CASES}
TIMES = {}                                                               # case id -> seconds (printed at the end of the module)


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _report_times():
    yield
    for k, v in TIMES.items():
        print("size-limit case %-28s %6.2f s" % (k, v))


class _Case(object):
    """`with _Case(id) as c:` -- skips when the row's declared peak does not fit, measures the wall time of the body."""

    def __init__(self, cid):
        self.c = CASES[cid]

    def __enter__(self):
        free, _total = torch.cuda.mem_get_info()
        if free < self.c.peak_bytes + (1 << 30):
            pytest.skip("%s declares a peak of %.1f GiB (+ 1 GiB for the allocator); %.1f GiB are free on this device"
                        % (self.c.id, self.c.peak_bytes / T.GiB, free / T.GiB))
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()
        return self.c

    def __exit__(self, exc_type, exc, tb):
        torch.cuda.synchronize()
        TIMES[self.c.id] = time.perf_counter() - self.t0
        if exc_type is None:
            peak = torch.cuda.max_memory_allocated()
            assert peak <= self.c.peak_bytes, "%s held %.2f GiB, the table declares %.2f" % (self.c.id, peak / T.GiB, self.c.peak_bytes / T.GiB)
        return False


FILL = 1 << 24


def hashed_range(a, b, lo, hi, salt, dtype=torch.float32, scale=1.0):
    """Elements [a, b) of the flat sequence v[i] = (lo + mix(i, salt) % (hi - lo + 1)) * scale: integer valued (or multiples of
    `scale`), a function of ALL bits of i (two 64-bit multiplications with a shift between them)."""
    h = torch.arange(a, b, dtype=torch.int64, device="cuda")
    h = (h + salt) * -7046029254386353131                                 # 0x9E3779B97F4A7C15 as a signed 64-bit integer
    h = (h ^ ((h >> 29) & 0x7FFFFFFFF)) * -4658895280553007687          # 0xBF58476D1CE4E5B9
    h = ((h >> 32) & 0x7FFFFFFF) % (hi - lo + 1) + lo
    return h.to(dtype) if scale == 1.0 else h.to(dtype) * scale


def hashed(shape, lo, hi, salt, dtype=torch.float32, scale=1.0):
    """A tensor of `shape` holding hashed_range over its flat index, filled in chunks."""
    n = 1
    for s in shape:
        n *= s
    out = torch.empty(n, dtype=dtype, device="cuda")
    for a in range(0, n, FILL):
        b = min(a + FILL, n)
        out[a:b] = hashed_range(a, b, lo, hi, salt, dtype, scale)
    return out.view(shape)


def check_chunks(got, ref_of, rows, what):
    """got: the whole output; ref_of(a, b) -> the expected got[a:b]; `rows` leading indices per chunk.  Every element is compared."""
    per_row = got[0].numel() if got.dim() > 1 else 1
    for a in range(0, got.shape[0], rows):
        b = min(a + rows, got.shape[0])
        ref = ref_of(a, b)
        assert ref.dtype == got.dtype, (ref.dtype, got.dtype)
        msg = lr.first_mismatch(got[a:b], ref, a * per_row, got.element_size())
        assert msg is None, "%s, rows [%d, %d): %s" % (what, a, b, msg)
        del ref


@pytest.mark.gpu
def test_no_two_images_and_no_two_positions_4_gib_apart_are_equal():
    x = hashed((5, 3, 64, 64), -8, 8, 1)
    assert len({bytes(img.cpu().numpy().tobytes()) for img in x}) == 5 and float(x.min()) == -8 and float(x.max()) == 8
    assert torch.equal(x, torch.round(x))
    a = hashed(((1 << 20) + 5,), -128, 127, 3)
    n = 1 << 18
    assert float((a[:n] == a[n:2 * n]).float().mean()) < 0.02           # a period of 2^18 would make every pair equal
    # ... and the chunked comparison sees ONE wrong element in the last, partial chunk and says where it is
    got = a.clone()
    got[-2] += 1
    with pytest.raises(AssertionError, match=r"1 of 5 elements of this chunk differ; first at flat index %d \(byte offset %d" % (a.numel() - 2, a.numel() * 4 - 8)):
        check_chunks(got, lambda lo, hi: a[lo:hi], n, "self-check")
    check_chunks(a, lambda lo, hi: a[lo:hi].clone(), n, "self-check")


# ---- float convolutions ------------------------------------------------------------------------------------------------------

def _conv_operands(c, cin, cout, r=1):
    """x in [-8, 8], w in [-8, 8], bias in [-50, 50]: |partial sums| <= r * r * cin * 64 + 50 < 2^24, so the fp32 matmul form of the
    reference and the kernel's own fp32 sum are both the exact integer."""
    assert r * r * cin * 64 + 50 < 1 << 24
    n, h, w = c.args[0], c.args[2], c.args[3]
    x = hashed((n, cin, h, w), -8, 8, 11)
    wt = hashed((cout, cin, r, r), -8, 8, 12)
    bias = hashed((cout,), -50, 50, 13)
    return x, wt, bias


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["c1_bit31", "c1_top_ktail", "c1_in_top"])
def test_conv1x1_f32_plain_and_abs_max(nat, cid):
    with _Case(cid) as c:
        n, cin, h, w, cout, stride = c.args
        x, wt, bias = _conv_operands(c, cin, cout)
        w2 = wt.view(cout, cin)
        mx = torch.zeros(2, device="cuda")
        y = nat.conv1x1_f32(x, w2.t().contiguous(), bias, stride, max_dev=mx, row=1)
        assert y.numel() * 4 == c.big_bytes or x.numel() * 4 == c.big_bytes
        per = max(1, (1 << 26) // y[0].numel())
        check_chunks(y, lambda a, b: lr.conv1x1_f32(x[a:b], w2, bias, stride), per, cid)
        assert float(mx[0]) == 0.0 and float(mx[1]) == float(lr.absmax(y))


@pytest.mark.gpu
def test_conv1x1_f32_top_row_in_every_form(nat):
    """63 x 16 x 127 x 129 -> 1036: 1 069 285 644 outputs (99.6 % of 2^30), 1 032 129 columns = 8063.5 tiles, 8.1 channel tiles.
    Plain; abs-max + ReLU copy; histogram + ReLU copy; the ReLU copy alone (out=False); QuanDequan."""
    cid = "c1_top"
    with _Case(cid) as c:
        n, cin, h, w, cout, stride = c.args
        x, wt, bias = _conv_operands(c, cin, cout)
        w2 = wt.view(cout, cin)
        wk = w2.t().contiguous()
        per = max(1, (1 << 26) // (cout * h * w))

        def ref(a, b):
            return lr.conv1x1_f32(x[a:b], w2, bias, stride)

        y = nat.conv1x1_f32(x, wk, bias, stride)
        check_chunks(y, ref, per, cid + " plain")
        want_max = lr.absmax(y)
        iv = 0.125                                                       # a power of two: the quotient is exact on any divider
        want_hist = torch.zeros(2048, dtype=torch.int64, device="cuda")
        for a in range(n):
            want_hist = lr.hist2048(y[a], iv, hist=want_hist)
        assert int(want_hist[2047]) > 0 and int(want_hist[8:16].sum()) > 0
        y.fill_(-1.0)
        r = torch.full_like(y, -1.0)
        mx = torch.zeros(1, device="cuda")
        nat.conv1x1_f32(x, wk, bias, stride, max_dev=mx, row=0, relu_out=r, out=y)
        check_chunks(y, ref, per, cid + " abs-max form, y")
        check_chunks(r, lambda a, b: lr.relu(ref(a, b)), per, cid + " abs-max form, ReLU copy")
        assert float(mx[0]) == float(want_max)
        y.fill_(-1.0)
        r.fill_(-1.0)
        ivd = torch.tensor([iv], device="cuda")
        hist = torch.ones(1, 2048, dtype=torch.int64, device="cuda")    # accumulated onto existing counts
        nat.conv1x1_f32(x, wk, bias, stride, interval_dev=ivd, hist_dev=hist, row=0, relu_out=r, out=y)
        check_chunks(y, ref, per, cid + " histogram form, y")
        check_chunks(r, lambda a, b: lr.relu(ref(a, b)), per, cid + " histogram form, ReLU copy")
        assert torch.equal(hist[0], want_hist + 1)
        r.fill_(-1.0)
        nat.conv1x1_f32(x, wk, bias, stride, relu_out=r, out=False)
        check_chunks(r, lambda a, b: lr.relu(ref(a, b)), per, cid + " ReLU copy alone")
        del r
        nat.conv1x1_f32(x, wk, bias, stride, out=y, qd=-3)
        check_chunks(y, lambda a, b: lr.quandequan(ref(a, b), -3), per, cid + " QuanDequan")
        # the split-bf16 form of the same layer: integers up to 8 are bf16 values, so its three-piece products are exact too
        y.fill_(-1.0)
        mx.zero_()
        nat.conv1x1_f32(x, nat.pack_sb_weight(w2), bias, stride, max_dev=mx, row=0, out=y)
        check_chunks(y, ref, per, cid + " split-bf16 form")
        assert float(mx[0]) == float(want_max)


@pytest.mark.gpu
def test_conv1x1_add_f32_top_row_with_everything_kept(nat):
    """fq_conv1x1_add_f32 and fq_conv1x1_add_hist_f32, fp32 and split-bf16, at 63 x 16 x 127 x 129 -> 1024 (1 056 900 096 outputs,
    98.4 % of 2^30): y, the sum and the ReLU are all written in the abs-max form, only the ReLU in the histogram form."""
    cid = "c1add_top"
    with _Case(cid) as c:
        n, cin, h, w, cout, stride = c.args
        x, wt, bias = _conv_operands(c, cin, cout)
        w2 = wt.view(cout, cin)
        res = hashed((n, cout, h, w), -500, 500, 14)
        per = max(1, (1 << 26) // (cout * h * w))

        def ref(a, b):
            return lr.conv1x1_f32(x[a:b], w2, bias, stride)

        y, sm, r = (torch.empty_like(res) for _ in range(3))
        ivd = torch.tensor([0.125, 0.25], device="cuda")
        want = None
        for form, wk in (("fp32", w2.t().contiguous()), ("split-bf16", nat.pack_sb_weight(w2))):
            what = "%s %s" % (cid, form)
            for t in (y, sm, r):
                t.fill_(-1.0)
            mx = torch.zeros(2, device="cuda")
            nat.conv1x1_add_f32(x, wk, bias, stride, res, mx, 0, 1, r, out=y, sum_out=sm)
            check_chunks(y, ref, per, what + ", y")
            check_chunks(sm, lambda a, b: ref(a, b) + res[a:b], per, what + ", sum")
            check_chunks(r, lambda a, b: lr.relu(ref(a, b) + res[a:b]), per, what + ", ReLU")
            assert float(mx[0]) == float(lr.absmax(y)) and float(mx[1]) == float(lr.absmax(sm))
            if want is None:
                want = torch.ones(2, 2048, dtype=torch.int64, device="cuda")
                for a in range(n):
                    want[0] = lr.hist2048(y[a], 0.125, hist=want[0])
                    want[1] = lr.hist2048(sm[a], 0.25, hist=want[1])
                assert int(want[0, 2047]) > 1 and int(want[1, 2047]) > 1
            r.fill_(-1.0)
            hist = torch.ones(2, 2048, dtype=torch.int64, device="cuda")
            nat.conv1x1_add_hist_f32(x, wk, bias, stride, res, ivd, hist, 0, 1, r)
            check_chunks(r, lambda a, b: lr.relu(ref(a, b) + res[a:b]), per, what + ", histogram form, ReLU")
            assert torch.equal(hist, want), what + ", histograms"


@pytest.mark.gpu
def test_conv_kxk_f32_top_row(nat):
    cid = "kxk_top"
    with _Case(cid) as c:
        n, cin, h, w, cout, r, s, stride, pad = c.args
        x, wt, bias = _conv_operands(c, cin, cout, r)
        mx = torch.zeros(1, device="cuda")
        y = nat.conv_kxk_f32(x, nat.pack_kxk_weight(wt), bias, (r, s), stride, pad, max_dev=mx, row=0)
        per = max(1, (1 << 26) // y[0].numel())
        check_chunks(y, lambda a, b: lr.conv_kxk_f32(x[a:b], wt, bias, stride, pad), per, cid)
        assert float(mx[0]) == float(lr.absmax(y))


@pytest.mark.gpu
def test_conv3x3_wino_f32_top_row(nat):
    """520 x 8 x 127 x 127 -> 64: y and its ReLU copy 2 147 092 480 bytes each (odd H and W: the single-pixel stores and the end-of-row
    loads).  Integer data keep the transformed weights multiples of 1/4 and every sum exact, so the result is the integer convolution."""
    cid = "wino_top"
    with _Case(cid) as c:
        n, cin, h, w, cout = c.args
        x, wt, bias = _conv_operands(c, cin, cout, 3)
        assert nat.conv_wino_supported(n, cin, h, w, cout) and not nat.conv_wino_supported(n + 1, cin, h, w, cout)
        relu = torch.full((n, cout, h, w), -1.0, device="cuda")
        mx = torch.zeros(1, device="cuda")
        y = nat.conv_wino_f32(x, nat.pack_wino_weight(wt), bias, cout, max_dev=mx, row=0, relu_out=relu)
        assert y.numel() * 4 == c.value

        def ref(a, b):
            return lr.conv_kxk_f32(x[a:b], wt, bias, 1, 1)

        check_chunks(y, ref, 32, cid)
        check_chunks(relu, lambda a, b: lr.relu(ref(a, b)), 32, cid + " ReLU copy")
        assert float(mx[0]) == float(lr.absmax(y))


@pytest.mark.gpu
def test_dwconv_f32_and_gconv_f32_top_rows(nat):
    """Odd 127 x 127 planes, 3x3, stride 1, padding 1, outputs at 99.9 % of 2^30: y, the ReLU copy and the abs-max."""
    for cid in ("dwf_top", "gf_top"):
        with _Case(cid) as c:
            if cid == "dwf_top":
                n, ch, h, w, r, s_, stride, pad = c.args
                k, groups = ch, ch
            else:
                n, ch, h, w, k, groups, r, s_, stride, pad = c.args
            assert r * s_ * (ch // groups) * 64 + 50 < 1 << 24
            x = hashed((n, ch, h, w), -8, 8, 191)
            wt = hashed((k, ch // groups, r, s_), -8, 8, 192)
            bias = hashed((k,), -50, 50, 193)
            relu = torch.full((n, k, h, w), -1.0, device="cuda")
            mx = torch.zeros(1, device="cuda")
            if cid == "dwf_top":
                y = nat.dwconv_f32(x, wt, bias, (r, s_), stride, pad, max_dev=mx, row=0, relu_out=relu)
            else:
                y = nat.gconv_f32(x, wt, bias, groups, (r, s_), stride, pad, max_dev=mx, row=0, relu_out=relu)
            assert y.numel() == c.value

            def ref(a, b):
                conv = lr.dwconv_taps(x[a:b], wt, stride, pad) if cid == "dwf_top" else lr.gconv_taps(x[a:b], wt, groups, stride, pad)
                return conv + bias.view(1, -1, 1, 1)

            per = max(1, (1 << 25) // y[0].numel())
            check_chunks(y, ref, per, cid)
            check_chunks(relu, lambda a, b: lr.relu(ref(a, b)), per, cid + " ReLU copy")
            assert float(mx[0]) == float(lr.absmax(y))
            del x, wt, y, relu
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_conv_stem_f32_resnet101_at_512_batch_255(nat):
    """The largest batch of ResNet-101 at 512 x 512 the stem takes: 255 x 64 x 256 x 256 outputs, y and its ReLU copy 4.0 GiB each."""
    cid = "stem_f32_r101_512_b255"
    with _Case(cid) as c:
        n, cin, h, w, cout, r, s, stride, pad = c.args
        x, wt, bias = _conv_operands(c, cin, cout, r)
        mx = torch.zeros(1, device="cuda")
        relu = torch.full((n, cout, 256, 256), -1.0, device="cuda")
        y = nat.conv_stem_f32(x, nat.pack_stem_weight(wt), bias, cout, (r, s), stride, pad, max_dev=mx, row=0, relu_out=relu)
        assert y.numel() == c.value

        def ref(a, b):
            return lr.conv_kxk_f32(x[a:b], wt, bias, stride, pad)

        check_chunks(y, ref, 8, cid)
        check_chunks(relu, lambda a, b: lr.relu(ref(a, b)), 8, cid + " ReLU copy")
        assert float(mx[0]) == float(lr.absmax(y))


# ---- float pooling and element-wise producers ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["pool_quad", "pool_generic"])
def test_maxpool2d_f32_beyond_2_31_input_elements(nat, cid):
    with _Case(cid) as c:
        planes, h, w, kh, kw, sh, sw, ph, pw = c.args
        x = hashed((planes // 4, 4, h, w), -1000, 1000, 21)
        assert x.numel() > 1 << 31
        y = nat.maxpool2d_f32(x, (kh, kw), (sh, sw), (ph, pw))
        check_chunks(y, lambda a, b: torch.nn.functional.max_pool2d(x[a:b], (kh, kw), (sh, sw), (ph, pw)), 64, cid)


@pytest.mark.gpu
def test_quandequan_and_add_sat_with_a_scalar_tail_beyond_2_31(nat):
    rows = 1 << 26
    with _Case("quandequan_flat") as c:
        x = hashed(c.args, -700, 700, 31, scale=0.25)                    # quarters: ties of the rounding at bit 1, saturation
        y = nat.quandequan(x, 1)
        check_chunks(y, lambda a, b: lr.quandequan(x[a:b], 1), rows, c.id)
        del x, y
    torch.cuda.empty_cache()
    with _Case("add_sat_flat") as c:
        a_ = hashed(c.args, -128, 127, 32)
        b_ = hashed(c.args, -128, 127, 33)
        y = nat.add_sat(a_, b_)
        check_chunks(y, lambda a, b: lr.add_sat(a_[a:b], b_[a:b]), rows, c.id)


def _bias_case(c):
    n, ch, hw = c.args
    y = hashed((n, ch, hw), -127, 127, 41)
    bias = hashed((ch,), -254, 254, 42)
    return y, bias, torch.full_like(y, -1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["bias_absmax_vec", "bias_absmax_odd"])
def test_bias_add_absmax_with_the_relu_copy_just_above_2_31(nat, cid):
    with _Case(cid) as c:
        y, bias, relu = _bias_case(c)
        mx = torch.full((1,), 0.5, device="cuda")
        nat.bias_add_absmax(y, bias, mx, 0, relu_out=relu)               # in place
        per = y[0].numel()

        def ref(a, b):                                                   # (the input again, from its hash)
            return hashed_range(a * per, b * per, -127, 127, 41).view(b - a, *y.shape[1:]) + bias.view(1, -1, 1)

        check_chunks(y, ref, 1, cid)
        check_chunks(relu, lambda a, b: lr.relu(ref(a, b)), 1, cid + " ReLU copy")
        assert float(mx[0]) == float(lr.absmax(y)) > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["bias_hist_vec", "bias_hist_odd"])
def test_bias_add_hist_with_the_relu_copy_just_above_2_31(nat, cid):
    with _Case(cid) as c:
        y, bias, relu = _bias_case(c)
        iv = 0.125                                                       # |y + b| <= 381: bins up to 2047 and the clamp beyond
        hist = torch.ones(1, 2048, dtype=torch.int64, device="cuda")
        nat.bias_add_hist(y, bias, torch.tensor([iv], device="cuda"), hist, 0, relu_out=relu)
        want = torch.ones(2048, dtype=torch.int64, device="cuda")
        for a in range(y.shape[0]):
            want = lr.hist2048(y[a], iv, hist=want)
        assert torch.equal(hist[0], want) and int(want[2047]) > 1 and int(want[8]) > 1
        per = y[0].numel()

        def ref(a, b):
            return hashed_range(a * per, b * per, -127, 127, 41).view(b - a, *y.shape[1:]) + bias.view(1, -1, 1)

        check_chunks(y, ref, 1, cid)
        check_chunks(relu, lambda a, b: lr.relu(ref(a, b)), 1, cid + " ReLU copy")


@pytest.mark.gpu
def test_add_absmax_and_add_hist_with_a_scalar_tail_beyond_2_31(nat):
    rows, hist_rows = 1 << 26, 1 << 25
    for cid in ("add_absmax_flat", "add_hist_flat"):
        with _Case(cid) as c:
            a_ = hashed(c.args, -127, 127, 51)
            b_ = hashed(c.args, -127, 127, 52)
            if cid == "add_absmax_flat":
                mx = torch.zeros(1, device="cuda")
                z = nat.add_absmax(a_, b_, mx, 0)
                assert float(mx[0]) == float(lr.absmax(z)) == 254.0
            else:
                iv = 0.125
                hist = torch.ones(1, 2048, dtype=torch.int64, device="cuda")
                z = nat.add_hist(a_, b_, torch.tensor([iv], device="cuda"), hist, 0)
                want = torch.ones(2048, dtype=torch.int64, device="cuda")
                for a in range(0, z.numel(), hist_rows):
                    want = lr.hist2048(z[a:a + hist_rows], iv, hist=want)
                assert torch.equal(hist[0], want) and int(want[2032]) > 1
            check_chunks(z, lambda a, b: a_[a:b] + b_[a:b], rows, cid)
            del a_, b_, z
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_absmax_seg_and_hist2048_seg_on_one_segment_beyond_2_31(nat):
    rows = 1 << 25
    with _Case("absmax_seg_flat") as c:
        x = hashed(c.args, -1000, 1000, 61)
        x[-1] = -1001.0                                                  # the maximum sits in the scalar tail
        mx = torch.tensor([0.0, 7.0, 2000.0], device="cuda")
        nat.absmax_seg([x], [1], mx)
        assert mx.tolist() == [0.0, 1001.0, 2000.0]
        nat.absmax_seg([x], [2], mx)
        assert mx.tolist() == [0.0, 1001.0, 2000.0]                      # folded into an existing, larger value
    with _Case("hist_seg_flat") as c:
        iv = torch.tensor([0.5, 0.25], device="cuda")                    # |x| / 0.25 <= 4004: every bin and the clamp; zeros are not counted
        hist = torch.ones(2, 2048, dtype=torch.int64, device="cuda")
        nat.hist2048_seg([x], [1], iv, hist)
        want = torch.ones(2048, dtype=torch.int64, device="cuda")
        zeros = 0
        for a in range(0, x.numel(), rows):
            want = lr.hist2048(x[a:a + rows], 0.25, hist=want)
            zeros += int((x[a:a + rows] == 0).sum())
        assert torch.equal(hist[1], want) and torch.equal(hist[0], torch.ones_like(want))
        assert int(want.sum()) - 2048 == x.numel() - zeros and zeros > 0 and int(want[2047]) > 1


# ---- dense int8 convolution on the register-staged tile kernel ---------------------------------------------------------------

OB = 3


def _logged(nat, variant, fn, *args):
    nat.conv_variant_log = log = {}
    try:
        out = fn(*args)
    finally:
        nat.conv_variant_log = None
    assert log == {variant: 1}, "ran %s, the table says %s" % (log, variant)
    return out


def _i8_operands(nat, c, wmax=127):
    """int8 NHWC x and weights from the hash; biases with the magnitudes of test_a_bias_far_outside_the_output_range...;
    |partial sums| <= R * S * C * 128 * (wmax + 1) < 2^24: the fp32 matmuls of the reference give the exact accumulator."""
    n, h, w, ch, k, r, s_ = c.args[:7]
    assert r * s_ * ch * 128 * (wmax + 1) < 1 << 24
    x = hashed((n, h, w, ch), -128, 127, 131, dtype=torch.int8)
    wq = hashed((k, ch, r, s_), -wmax - 1, wmax, 132)
    if (r, s_) == (1, 1):
        wq = wq.view(k, ch)
    qb = hashed((k,), -128, 127, 133)
    qb[::7] = torch.tensor([300.0, -1e5, 3e9, -40000.0, 255.0, -256.0], device="cuda").repeat(k // 42 + 1)[:len(qb[::7])]
    return x, wq, nat.pack_weight_krsc(wq.view(k, ch, r, s_)), qb


def _acc_kxk(x, wq, a, b, stride, pad):
    """the exact accumulator of images [a, b) of an R x S layer as fp32 [n][K][P*Q], tap by tap"""
    xf = x[a:b].permute(0, 3, 1, 2).to(torch.float32)
    acc = lr.conv_kxk_f32(xf, wq, torch.zeros(wq.shape[0], device="cuda"), stride, pad)
    return acc.view(acc.shape[0], acc.shape[1], -1)


def _acc(x, wq, a, b):
    """the exact accumulator of images [a, b) as fp32 [n][K][H*W]"""
    n, h, w, ch = x[a:b].shape
    return torch.matmul(wq, x[a:b].reshape(n, h * w, ch).to(torch.float32).transpose(1, 2))


def _nhwc(t, kpad):
    """[n][K][HW] integer valued -> [n][HW][kpad] with zeros in the padding channels (what the kernels must leave there)"""
    n, k, hw = t.shape
    out = torch.zeros((n, hw, kpad), dtype=t.dtype, device=t.device)
    out[..., :k] = t.transpose(1, 2)
    return out


GEOM = ((1, 1), (0, 0), (1, 1))


@pytest.mark.gpu
def test_conv2d_i8_input_just_below_2_31_bytes(nat):
    cid = "i8_in_top_k16"
    with _Case(cid) as c:
        n, h, w, ch, k = c.args[:5]
        x, wq, wk, qb = _i8_operands(nat, c)
        assert x.numel() == c.value
        rs = 10
        y, q = _logged(nat, "tile_general/64", nat.conv2d_i8_resident, x, wk, qb, *GEOM, rs, OB, True, True, True)

        def ref(a, b):
            return lr.relu(lr.recon_epilogue(_acc(x, wq, a, b), qb, rs, OB))

        check_chunks(y.view(n, k, h * w), ref, 8, cid + " fp32 NCHW")
        check_chunks(q.view(n, h * w, 16), lambda a, b: _nhwc(lr.quantity(ref(a, b), OB).to(torch.int8), 16), 8, cid + " int8 NHWC")


@pytest.mark.gpu
def test_conv2d_i8_input_top_with_64_output_channels(nat):
    """255 x 128 x 256 x 256 -> 64, 1x1, int8 output: the C % 128 == 0 path of the register-staged tile kernel with 64-row tiles (the
    streaming 1x1 kernel that would also take this layer is opt-in, FQ_CONV_STREAM=1, and rows name the kernel reached without a
    switch); and the fused-add form with an int16 residual, wide and narrow outputs."""
    cid = "i8_in_top_k64"
    with _Case(cid) as c:
        n, h, w, ch, k = c.args[:5]
        x, wq, wk, qb = _i8_operands(nat, c)
        rs, hw = 11, h * w
        _y, q = _logged(nat, "tile_c128/64", nat.conv2d_i8_resident, x, wk, qb, *GEOM, rs, OB, False, True, True)

        def tail(a, b, ob=OB):
            return lr.recon_epilogue(_acc(x, wq, a, b), qb, rs, ob)

        check_chunks(q.view(n, hw, k), lambda a, b: _nhwc(lr.quantity(lr.relu(tail(a, b)), OB).to(torch.int8), k), 4, cid + " int8 NHWC")
        del q
        g_res, ib = 6, 4
        res = hashed((n, hw, k), -128 << g_res, (128 << g_res) - 1, 146, dtype=torch.int16)
        wide, narrow = _logged(nat, "tile_c128/64", nat.conv2d_i8_add_resident, x, wk, qb, *GEOM, rs, OB, res.view(n, h, w, k), g_res, True, g_res,
                               True, ib, False)

        def both(a, b):
            return lr.add_resident(tail(a, b, ob=0), OB, res[a:b].transpose(1, 2), g_res, g_res, ib, False)

        check_chunks(wide.view(n, hw, k), lambda a, b: _nhwc(both(a, b)[0], k), 4, cid + " fused add, wide")
        check_chunks(narrow.view(n, hw, k), lambda a, b: _nhwc(both(a, b)[1], k), 4, cid + " fused add, narrow")


@pytest.mark.gpu
def test_conv2d_i8_input_top_on_the_lds_dma_kernel(nat):
    """255 x 128 x 256 x 256 -> 64, 3x3, stride 2, padding 1: conv2d_i8_dma with a ring of two, int8 and fp32 outputs."""
    cid = "i8_in_top_3x3s2"
    with _Case(cid) as c:
        n, h, w, ch, k, r, s_, stride, pad = c.args
        x, wq, wk, qb = _i8_operands(nat, c, wmax=63)
        rs, pq = 13, (h // 2) * (w // 2)
        y, q = _logged(nat, "dma2/64", nat.conv2d_i8_resident, x, wk, qb, (stride, stride), (pad, pad), (1, 1), rs, OB, True, True, False)

        def tail(a, b):
            return lr.recon_epilogue(_acc_kxk(x, wq, a, b, stride, pad), qb, rs, OB)

        check_chunks(y.view(n, k, pq), tail, 4, cid + " fp32 NCHW")
        check_chunks(q.view(n, pq, k), lambda a, b: _nhwc(lr.quantity(tail(a, b), OB).to(torch.int8), k), 4, cid + " int8 NHWC")


@pytest.mark.gpu
def test_conv2d_i8_input_top_on_the_stationary_64_channel_kernel(nat):
    """8454 x 64 x 63 x 63 -> 64, 3x3 / 1 / 1: conv3x3_i8_c64 (persistent workgroups over 262 141.9 pixel tiles, input slabs of
    130 + 2 W pixel rows through LDS-DMA with `pixel * 64` as a 32-bit byte offset), fp32 output of 8.6 GB."""
    cid = "i8_in_top_c64"
    with _Case(cid) as c:
        n, h, w, ch, k, r, s_, stride, pad = c.args
        x, wq, wk, qb = _i8_operands(nat, c)
        rs = 12
        y = _logged(nat, "c64_halo/64", nat.conv2d_i8, x, wk, qb, (stride, stride), (pad, pad), (1, 1), rs, OB)
        assert x.numel() == c.value and y.numel() * 4 == c.big_bytes
        check_chunks(y.view(n, k, h * w), lambda a, b: lr.recon_epilogue(_acc_kxk(x, wq, a, b, stride, pad), qb, rs, OB), 128, cid)


@pytest.mark.gpu
def test_conv2d_i8_outputs_just_below_2_30_elements(nat):
    """79 x 16 x 255 x 255 -> 200 (Kpad 208): M * Kpad = 1 068 490 800, 40 132.6 pixel tiles, 1.6 channel tiles; int8 + fp32; the fused
    add with an int8 and an int16 residual, wide and narrow outputs; per-channel shifts."""
    cid = "i8_out_top"
    with _Case(cid) as c:
        n, h, w, ch, k = c.args[:5]
        kpad, hw = T.pad16(k), h * w
        x, wq, wk, qb = _i8_operands(nat, c)
        assert n * hw * kpad == c.value
        rs, var = 8, "tile_general/128"

        def tail(a, b, shift=rs, ob=OB):
            return lr.recon_epilogue(_acc(x, wq, a, b), qb, shift, ob)

        y, q = _logged(nat, var, nat.conv2d_i8_resident, x, wk, qb, *GEOM, rs, OB, True, True, False)
        check_chunks(y.view(n, k, hw), tail, 2, cid + " fp32 NCHW")
        check_chunks(q.view(n, hw, kpad), lambda a, b: _nhwc(lr.quantity(tail(a, b), OB).to(torch.int8), kpad), 2, cid + " int8 NHWC")
        del y, q
        ib = 4
        for res_dtype, g_res, relu, want_wide in ((torch.int8, 5, True, True), (torch.int16, 6, False, True), (torch.int8, 2, True, False)):
            what = "%s fused add, %s residual g_res=%d relu=%d wide=%d" % (cid, res_dtype, g_res, relu, want_wide)
            lim = 128 << g_res if res_dtype == torch.int16 else 128
            res = hashed((n, hw, kpad), -lim, lim - 1, 140 + g_res, dtype=res_dtype)
            res[..., k:] = 0
            g = max(0, OB, g_res)
            wide, narrow = _logged(nat, var, nat.conv2d_i8_add_resident, x, wk, qb, *GEOM, rs, OB, res.view(n, h, w, kpad), g_res,
                                   want_wide, g, True, ib, relu)

            def both(a, b):
                conv_q = tail(a, b, ob=0)                                # the integers, value conv_q * 2^-OB
                return lr.add_resident(conv_q, OB, res[a:b, :, :k].transpose(1, 2), g_res, g, ib, relu)

            assert (wide is not None) == want_wide
            if want_wide:
                check_chunks(wide.view(n, hw, kpad), lambda a, b: _nhwc(both(a, b)[0], kpad), 2, what + ", wide")
            check_chunks(narrow.view(n, hw, kpad), lambda a, b: _nhwc(both(a, b)[1], kpad), 2, what + ", narrow")
            del res, wide, narrow
        shifts = (torch.arange(k, device="cuda") * 5 % 9 + rs - 4).to(torch.int32)      # rs - 4 .. rs + 4, both ends present
        vec = nat.ShiftVec(shifts, rs - 4, rs + 4)
        y = _logged(nat, var, nat.conv2d_i8, x, wk, qb, *GEOM, vec, OB)
        check_chunks(y.view(n, k, hw), lambda a, b: lr.pc_epilogue(_acc(x, wq, a, b), qb, shifts, OB), 2, cid + " per-channel shifts")


@pytest.mark.gpu
def test_conv2d_i8_fp32_output_beyond_4_gib(nat):
    cid = "i8_f32_4gib"
    with _Case(cid) as c:
        n, h, w, ch, k = c.args[:5]
        x, wq, wk, qb = _i8_operands(nat, c)
        y = _logged(nat, "tile_general/64", nat.conv2d_i8, x, wk, qb, *GEOM, 8, OB)
        assert y.numel() * 4 == c.big_bytes > 1 << 32
        check_chunks(y.view(n, k, h * w), lambda a, b: lr.recon_epilogue(_acc(x, wq, a, b), qb, 8, OB), 8, cid)


# ---- the block tails at the top ----------------------------------------------------------------------------------------------

def _bt_chain(x, w3, b3, rs3, ob3, res_of, g_res, g_wide, ib, w1, b1, rs1, a, b):
    """conv3 -> tail | + shortcut | clamp | ReLU | the wide sum and the next Quantity | conv1 -> tail -> ReLU for images [a, b), as
    tests/test_gpu_block_tail.py states the chain with the oracle: (wide, narrow, q1) as [n][HW][channels]."""
    conv_q = lr.recon_epilogue(_acc(x, w3, a, b), b3, rs3, 0)                       # the integers, value conv_q * 2^-ob3
    wide, narrow = lr.add_resident(conv_q, ob3, res_of(a, b), g_res, g_wide, ib, True)
    q1 = lr.relu(lr.recon_epilogue(torch.matmul(w1, narrow.to(torch.float32)), b1, rs1, 0)).to(torch.int8)
    return wide.transpose(1, 2).contiguous(), narrow.transpose(1, 2).contiguous(), q1.transpose(1, 2).contiguous()


def _bt_operands(nat, n, h, w, ch, k3, c2):
    assert ch * (1 << 14) < 1 << 24 and k3 * (1 << 14) < 1 << 24                  # both matmuls of the reference are exact
    x = hashed((n, h, w, ch), -128, 127, 201, dtype=torch.int8)
    w3 = hashed((k3, ch), -128, 127, 202)
    w1 = hashed((c2, k3), -128, 127, 203)
    b3, b1 = hashed((k3,), -100, 100, 204), hashed((c2,), -100, 100, 205)
    return x, w3, w1, b3, b1, nat.pack_weight_krsc(w3.view(k3, ch, 1, 1)), nat.pack_weight_krsc(w1.view(c2, k3, 1, 1))


@pytest.mark.gpu
def test_block_tail_i8_outputs_just_below_2_30_elements(nat):
    cid = "bt_top"
    with _Case(cid) as c:
        n, h, w, ch, k3, c2 = c.args
        hw, rs3, ob3, g_res, ib, rs1 = h * w, 9, 4, 5, 4, 11
        x, w3, w1, b3, b1, w3k, w1k = _bt_operands(nat, n, h, w, ch, k3, c2)
        res = hashed((n, hw, k3), -128 << g_res, (128 << g_res) - 1, 206, dtype=torch.int16)
        assert n * hw * k3 == c.value
        wide, narrow, q1 = _logged(nat, "block_tail/128", nat.block_tail_i8, x, w3k, b3, rs3, ob3, res.view(n, h, w, k3), g_res, True, 5,
                                   True, ib, True, w1k, b1, rs1, True)

        def ref(a, b):
            return _bt_chain(x, w3, b3, rs3, ob3, lambda a_, b_: res[a_:b_].transpose(1, 2), g_res, 5, ib, w1, b1, rs1, a, b)

        check_chunks(wide.view(n, hw, k3), lambda a, b: ref(a, b)[0], 4, cid + " wide")
        check_chunks(narrow.view(n, hw, k3), lambda a, b: ref(a, b)[1], 4, cid + " narrow")
        check_chunks(q1.view(n, hw, c2), lambda a, b: ref(a, b)[2], 4, cid + " next conv1")
        assert int((q1 != 0).sum()) > 0


@pytest.mark.gpu
def test_block_tail_proj_i8_outputs_just_below_2_30_elements(nat):
    cid = "btp_top"
    with _Case(cid) as c:
        n, h, w, ch, k3, c2, cp, sp, hp, wp_ = c.args
        hw, rs3, ob3, obp, rsp, ib, rs1 = h * w, 9, 4, 4, 8, 4, 11
        x, w3, w1, b3, b1, w3k, w1k = _bt_operands(nat, n, h, w, ch, k3, c2)
        xp = hashed((n, hp, wp_, cp), -128, 127, 207, dtype=torch.int8)
        wpq, bp = hashed((k3, cp), -128, 127, 208), hashed((k3,), -100, 100, 209)
        narrow, q1 = _logged(nat, "block_tail_proj/128", nat.block_tail_proj_i8, x, w3k, b3, rs3, ob3, xp, nat.pack_weight_krsc(wpq.view(k3, cp, 1, 1)),
                             bp, rsp, obp, sp, False, 4, True, ib, True, w1k, b1, rs1, True)[1:]

        def shortcut(a, b):                                              # the projection: 1x1 at stride 2, its own tail, no ReLU
            xs = xp[a:b, ::sp, ::sp].reshape(b - a, hw, cp).to(torch.float32).transpose(1, 2)
            return lr.recon_epilogue(torch.matmul(wpq, xs), bp, rsp, 0)

        def ref(a, b):
            return _bt_chain(x, w3, b3, rs3, ob3, shortcut, obp, 4, ib, w1, b1, rs1, a, b)

        check_chunks(narrow.view(n, hw, k3), lambda a, b: ref(a, b)[1], 4, cid + " narrow")
        check_chunks(q1.view(n, hw, c2), lambda a, b: ref(a, b)[2], 4, cid + " next conv1")
        assert int((q1 != 0).sum()) > 0


# ---- the concatenation kernels at the top ------------------------------------------------------------------------------------

def _cat_ref(srcs, a, b, cpad_out, relu_all):
    """The index rule of include/fq.h in torch for images [a, b): srcs = [(int8 NHWC tensor, C, up, relu)]."""
    parts = []
    for t, ch, up, relu in srcs:
        v = t[a:b, :, :, :ch]
        if up > 1:
            v = v.repeat_interleave(up, dim=1).repeat_interleave(up, dim=2)
        parts.append(v.clamp_min(0) if (relu or relu_all) else v)
    n, h, w = parts[-1].shape[:3]
    out = torch.zeros((n, h, w, cpad_out), dtype=torch.int8, device="cuda")
    out[..., :sum(p.shape[3] for p in parts)] = torch.cat(parts, dim=3)
    return out


def _cat_sources(c, relus):
    n, h, w = c.args[:3]
    srcs = []
    for i, relu in enumerate(relus):
        ch, up = c.args[3 + 2 * i], c.args[4 + 2 * i]
        srcs.append((hashed((n, h // up, w // up, T.pad16(ch)), -128, 127, 150 + i, dtype=torch.int8), ch, up, relu))   # garbage in the padding
    return srcs


@pytest.mark.gpu
def test_concat_i8_nhwc_output_just_below_2_31_bytes(nat):
    cid = "cat_top"
    with _Case(cid) as c:
        srcs = _cat_sources(c, (False, False))
        for relu in (True, False):
            out = nat.concat_i8_nhwc([(t, ch, up) for t, ch, up, _r in srcs], relu)
            assert out.numel() == c.value
            check_chunks(out, lambda a, b: _cat_ref(srcs, a, b, 64, relu), 16, "%s relu=%d" % (cid, relu))
            del out


@pytest.mark.gpu
def test_concat_n_i8_nhwc_output_just_below_2_31_bytes(nat):
    cid = "catn_top"
    with _Case(cid) as c:
        srcs = _cat_sources(c, (True, False, False))
        out = nat.concat_n_i8_nhwc(srcs)
        assert out.numel() == c.value
        check_chunks(out, lambda a, b: _cat_ref(srcs, a, b, 64, False), 16, cid)


@pytest.mark.gpu
def test_dwconv2d_i8_output_just_below_2_30_elements(nat):
    cid = "dwi_top"
    with _Case(cid) as c:
        n, h, w, ch, r, s_, stride, pad = c.args
        cpad, rs = T.pad16(ch), 9
        x = hashed((n, h, w, cpad), -128, 127, 161, dtype=torch.int8)      # garbage in the 13 padding channels
        wq = hashed((ch, 1, r, s_), -128, 127, 162)
        qb = hashed((ch,), -100, 100, 163)
        assert r * s_ * (1 << 14) < 1 << 24
        q = _logged(nat, "depthwise", nat.dwconv2d_i8_resident, x, nat.pack_weight_dw(wq), qb, (stride, stride), (pad, pad), rs, OB, True)
        assert q.numel() == c.value

        def ref(a, b):
            acc = lr.dwconv_taps(x[a:b, :, :, :ch].permute(0, 3, 1, 2).to(torch.float32), wq, stride, pad)
            out = torch.zeros((b - a, h, w, cpad), dtype=torch.int8, device="cuda")
            out[..., :ch] = lr.relu(lr.recon_epilogue(acc, qb, rs, 0)).to(torch.int8).permute(0, 2, 3, 1)
            return out

        check_chunks(q, ref, 64, cid)


@pytest.mark.gpu
def test_gconv2d_i8_output_just_below_2_30_elements(nat):
    cid = "gci_top"
    with _Case(cid) as c:
        n, h, w, ch, k, groups, r, s_, stride, pad = c.args
        cpad, kpad, rs = T.pad16(ch), T.pad16(k), 10
        x = hashed((n, h, w, cpad), -128, 127, 181, dtype=torch.int8)
        x[..., ch:] = 0
        wq = hashed((k, ch // groups, r, s_), -128, 127, 182)
        qb = hashed((k,), -100, 100, 183)
        assert r * s_ * (ch // groups) * (1 << 14) < 1 << 24
        q = _logged(nat, "grouped", nat.gconv2d_i8_resident, x, nat.pack_weight_grouped(wq, groups), qb, k, groups, (stride, stride),
                    (pad, pad), rs, OB, True)
        assert q.numel() == c.value

        def ref(a, b):
            acc = lr.gconv_taps(x[a:b, :, :, :ch].permute(0, 3, 1, 2).to(torch.float32), wq, groups, stride, pad)
            out = torch.zeros((b - a, h, w, kpad), dtype=torch.int8, device="cuda")
            out[..., :k] = lr.relu(lr.recon_epilogue(acc, qb, rs, 0)).to(torch.int8).permute(0, 2, 3, 1)
            return out

        check_chunks(q, ref, 32, cid)


@pytest.mark.gpu
def test_avgpool_i8_nhwc_source_just_below_2_31_bytes(nat):
    """3x3 / 1 / 1 on 4160 planes of 127 x 127 x 32 bytes, with and without count_include_pad: integer window sums, ONE fp32 division
    by the tap count (a device tensor: correctly rounded), the power of two, rint, the clamp; zeros in the padding channels."""
    cid = "avgi_top"
    with _Case(cid) as c:
        n, h, w, ch, kh, kw, sh, sw, ph, pw = c.args
        cpad = T.pad16(ch)
        x = hashed((n, h, w, cpad), -128, 127, 171, dtype=torch.int8)
        assert x.numel() == c.value and (kh, kw, sh, sw, ph, pw) == (3, 3, 1, 1, 1, 1)
        ones = torch.nn.functional.pad(torch.ones((1, h, w, 1), dtype=torch.int32, device="cuda"), (0, 0, 1, 1, 1, 1))
        taps = sum(ones[:, a:a + h, b:b + w] for a in range(3) for b in range(3)).to(torch.float32)
        for cip, shift, relu in ((False, 1, True), (True, 0, False)):
            y = nat.avgpool_i8_nhwc(x, ch, (kh, kw), (sh, sw), (ph, pw), cip, shift, relu)
            div = torch.full_like(taps, 9.0) if cip else taps

            def ref(a, b):
                xp = torch.nn.functional.pad(x[a:b, :, :, :ch].to(torch.int32), (0, 0, 1, 1, 1, 1))
                sums = sum(xp[:, i:i + h, j:j + w] for i in range(3) for j in range(3)).to(torch.float32)
                v = torch.round(sums / div * float(2 ** shift)).clamp(0.0 if relu else -128.0, 127.0)
                out = torch.zeros((b - a, h, w, cpad), dtype=torch.int8, device="cuda")
                out[..., :ch] = v.to(torch.int8)
                return out

            check_chunks(y, ref, 64, "%s count_include_pad=%d" % (cid, cip))
            del y


# ---- int8 kernels with an operand above 2^31 bytes --------------------------------------------------------------------------

@pytest.mark.gpu
def test_conv2d_i8_stem_with_2_18_gb_of_output(nat):
    cid = "stem_i8_b520"
    with _Case(cid) as c:
        n, cin, h, w, k, r, s, stride, pad = c.args
        ib, rs, ob = 1, 9, 3
        x = hashed((n, cin, h, w), -300, 300, 71, scale=0.25)            # x * 2^ib in halves: ties, and saturation at +-128
        wq = hashed((k, cin, r, s), -127, 127, 72)
        qb = hashed((k,), -100, 100, 73)
        assert r * s * cin * 128 * 127 < 1 << 24                         # the fp32 matmul form of the reference is exact
        nat.conv_variant_log = log = {}
        try:
            q = nat.conv2d_i8_stem(x, nat.pack_weight_stem(wq), qb, k, s, (stride, stride), (pad, pad), ib, rs, ob, True)
        finally:
            nat.conv_variant_log = None
        assert len(log) == 1 and next(iter(log)).startswith("stem"), log
        assert q.numel() == c.big_bytes and tuple(q.shape) == (n, 256, 256, 64)
        zero_b = torch.zeros(k, device="cuda")

        def ref(a, b):
            acc = lr.conv_kxk_f32(lr.quantity(x[a:b], ib), wq, zero_b, stride, pad)
            return lr.relu(lr.recon_epilogue(acc, qb, rs, 0)).to(torch.int8).permute(0, 2, 3, 1).contiguous()

        check_chunks(q, ref, 8, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["maxpool_i8_banded", "maxpool_i8_generic"])
def test_maxpool_i8_nhwc_with_an_input_above_2_31_bytes(nat, cid):
    with _Case(cid) as c:
        n, h, w, ch, kh, kw, sh, sw, ph, pw = c.args
        x = hashed((n, h, w, ch), -128, 127, 81, dtype=torch.int8)
        assert x.numel() == c.big_bytes > 1 << 31
        y = nat.maxpool_i8_nhwc(x, (kh, kw), (sh, sw), (ph, pw))
        check_chunks(y, lambda a, b: lr.maxpool_nhwc(x[a:b], (kh, kw), (sh, sw), (ph, pw)), 32, cid)


@pytest.mark.gpu
def test_add_resident_with_int16_operands_above_2_31_bytes(nat):
    cid = "add_resident_i16"
    with _Case(cid) as c:
        n = c.args[0]
        gx, gy, ib = 6, 8, 4
        x = hashed((n // 16, 16), -128 << gx, (128 << gx) - 1, 91, dtype=torch.int16)
        y = hashed((n // 16, 16), -128 << gy, (128 << gy) - 1, 92, dtype=torch.int16)
        assert x.numel() * 2 == c.big_bytes
        wide, narrow = nat.add_resident(x, gx, y, gy, True, 8, True, ib, True)
        rows = 1 << 22
        check_chunks(wide, lambda a, b: lr.add_resident(x[a:b], gx, y[a:b], gy, 8, ib, True)[0], rows, cid + " wide")
        check_chunks(narrow, lambda a, b: lr.add_resident(x[a:b], gx, y[a:b], gy, 8, ib, True)[1], rows, cid + " narrow")


@pytest.mark.gpu
def test_dequant_nhwc_to_nchw_with_more_than_2_30_outputs(nat):
    cid = "dequant_2_30"
    with _Case(cid) as c:
        n, ch, hw, cpad = c.args
        q = hashed((n, hw, 1, cpad), -128, 127, 101, dtype=torch.int8)
        y = nat.dequant_nhwc_to_nchw(q, 3, ch)
        assert y.numel() > 1 << 30 and tuple(y.shape) == (n, ch, hw, 1)
        check_chunks(y, lambda a, b: lr.dequant_nhwc_to_nchw(q[a:b], 3, ch), 8, cid)


@pytest.mark.gpu
def test_avgpool_global_nhwc_with_an_input_above_2_31_bytes(nat):
    cid = "avgpool_global_i16"
    with _Case(cid) as c:
        n, ch, hw, cpad = c.args
        q = hashed((n, hw, 1, cpad), -32768, 32767, 111, dtype=torch.int16)
        assert q.numel() * 2 == c.big_bytes
        y = nat.avgpool_global_nhwc(q, 8, ch)
        check_chunks(y.view(n, ch), lambda a, b: lr.avgpool_global_nhwc(q[a:b], 8, ch), 32, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["quantize_general_vec", "quantize_general_odd", "quantize_rows", "quantize_smallc"])
def test_quantize_i8_nhwc_with_an_input_above_2_31_elements(nat, cid):
    with _Case(cid) as c:
        n, ch, hw, cpad = c.args
        x = hashed((n, ch, hw, 1), -300, 300, 121, scale=0.25)
        assert x.numel() > 1 << 31
        q = nat.quantize_i8_nhwc(x, 1, cpad)
        assert tuple(q.shape) == (n, hw, 1, cpad)
        rows = max(1, (1 << 26) // (ch * hw))
        check_chunks(q, lambda a, b: lr.quantize_i8_nhwc(x[a:b], 1, cpad), rows, cid)
