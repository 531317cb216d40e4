"""The host-side size guards of libfq_hip.so, on a box without a GPU.

Every kernel indexes with 32 bits somewhere and its entry point refuses (FQ_ERR_UNSUPPORTED, -4) what does not fit, before any HIP
call: the library loads without a device and a refusal needs none.  tests/size_limit_cases.py lists per guard the first value it
refuses; each is passed through ctypes here with small aligned host buffers as pointers.  A guard loosened by one step admits its
row, the call goes on to a launch that has no device, and the status is no longer -4.

NEVER an admitted size in this file: it would launch.  And the whole module is skipped where a GPU is present -- a guard that
fails to refuse must not be able to launch a 10^9-element kernel over 4 KB buffers on a shared card.
"""
import ctypes
import os
import re

import pytest
import torch

import size_limit_cases as T

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def L():
    from common.quantity import _native
    return _native.lib()


@pytest.fixture(scope="module")
def buf():
    """(64-byte aligned pointer into a 4 KB host buffer, a second one 2 KB behind it)"""
    raw = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(raw) + 63) & ~63
    return ctypes.c_void_p(base), ctypes.c_void_p(base + 2048), raw


def _cat(L, struct, srcs, p):
    arr = (struct * len(srcs))()
    for i, (c, cpad, up) in enumerate(srcs):
        arr[i].q, arr[i].C, arr[i].Cpad, arr[i].up = p.value, c, cpad, up
    return arr


def _call(L, buf, entry, a):
    from common.quantity import _native
    p, p2, _raw = buf
    z = None
    if entry in ("fq_conv1x1_f32", "fq_conv1x1_sb_f32"):
        return getattr(L, entry)(p, p, p, p, z, *a, z, z, z, z, 0, z)
    if entry == "fq_conv_kxk_f32":
        return L.fq_conv_kxk_f32(p, p, p, p, z, *a, z, z, z, z, 0, z)
    if entry in ("fq_conv1x1_add_f32", "fq_conv1x1_sb_add_f32"):
        return getattr(L, entry)(p, p, p, p, p, p, p, *a, p, p2, z, 0, z)
    if entry == "fq_conv1x1_add_hist_f32":
        return L.fq_conv1x1_add_hist_f32(p, p, p, p, p, *a, p, p, p, p2, z, 0, z)
    if entry in ("fq_conv1x1_sb_pack", "fq_conv3x3_wino_f32_pack"):
        return getattr(L, entry)(p, p, *a, z)
    if entry == "fq_conv_stem_f32":
        return L.fq_conv_stem_f32(p, p, p, p, z, *a, z, z, z, z)
    if entry == "fq_conv3x3_wino_f32":
        return L.fq_conv3x3_wino_f32(p, p, p, p, z, *a, z, z, z, z)
    if entry in ("fq_dwconv_f32", "fq_gconv_f32"):
        return getattr(L, entry)(p, p, p, p, z, *a, z, z, z, z)
    if entry == "fq_maxpool2d_f32":
        return L.fq_maxpool2d_f32(p, p, *a, z)
    if entry == "fq_bias_add_absmax_f32":
        return L.fq_bias_add_absmax_f32(p, p, *a, p, z, z)
    if entry == "fq_bias_add_hist_f32":
        return L.fq_bias_add_hist_f32(p, p, *a, p, p, z, z)
    if entry in ("fq_absmax_chan", "fq_hist2048_chan"):
        seg = _native._ChanSeg(p.value, a[0], a[1], a[2], 0, 0)
        if entry == "fq_absmax_chan":
            return L.fq_absmax_chan(ctypes.byref(seg), 1, p, z)
        return L.fq_hist2048_chan(ctypes.byref(seg), 1, p, p2, z)
    if entry == "fq_hist2048_chain_seg":
        seg = _native._ChainSeg()
        seg.head, seg.n, seg.len = p.value, a[0], 1
        seg.y[0], seg.row_y[0], seg.row_sum[0] = p.value, 0, 1
        return L.fq_hist2048_chain_seg(ctypes.byref(seg), 1, p, p2, z)
    if entry == "fq_quantize_i8_nhwc":
        return L.fq_quantize_i8_nhwc(p, p, *a, 0, z)
    if entry in ("fq_dequant_nhwc_to_nchw", "fq_avgpool_global_nhwc"):
        return getattr(L, entry)(p, 1, 3, p, *a, z)
    if entry in ("fq_conv2d_i8", "fq_conv2d_i8_resident", "fq_conv2d_i8_add_resident"):
        N, H, W, C, K, R, S, st, pd = a
        geo = (N, H, W, C, K, R, S, st, st, pd, pd, 1, 1)
        if entry == "fq_conv2d_i8":
            return L.fq_conv2d_i8(p, p, p, p, *geo, 9, 3, 8, z)
        if entry == "fq_conv2d_i8_resident":
            return L.fq_conv2d_i8_resident(p, p, p, z, p, T.pad16(K), 0, *geo, 9, 3, z)
        return L.fq_conv2d_i8_add_resident(p, p, p, p, 1, 3, p, 3, p, 3, 0, T.pad16(K), *geo, 9, 3, z)
    if entry == "fq_dwconv2d_i8_resident":
        N, H, W, C, R, S, st, pd = a
        return L.fq_dwconv2d_i8_resident(p, p, p, p, T.pad16(C), 0, N, H, W, C, R, S, st, st, pd, pd, 1, 1, 9, 3, z)
    if entry == "fq_gconv2d_i8_resident":
        N, H, W, C, K, G, R, S, st, pd = a
        return L.fq_gconv2d_i8_resident(p, p, p, p, T.pad16(C), T.pad16(K), 0, N, H, W, C, K, G, R, S, st, st, pd, pd, 1, 1, 9, 3, z)
    if entry == "fq_avgpool_i8_nhwc":
        N, H, W, C, kh, kw, sh, sw, ph, pw = a
        return L.fq_avgpool_i8_nhwc(p, p, N, H, W, C, T.pad16(C), kh, kw, sh, sw, ph, pw, 0, 0, 0, z)
    if entry in ("fq_concat_i8_nhwc", "fq_concat_n_i8_nhwc"):
        N, H, W, c0, cp0, u0, c1, cp1, u1 = a
        cpad_out = T.pad16(c0 + c1)
        if entry == "fq_concat_i8_nhwc":
            return L.fq_concat_i8_nhwc(_cat(L, _native._CatSrc, [(c0, cp0, u0), (c1, cp1, u1)], p), 2, p, cpad_out, 1, N, H, W, z)
        return L.fq_concat_n_i8_nhwc(_cat(L, _native._CatSrcN, [(c0, cp0, u0), (c1, cp1, u1)], p), 2, p, cpad_out, N, H, W, z)
    if entry == "fq_block_tail_i8":
        M, C, K3, C2 = a
        return L.fq_block_tail_i8(p, p, p, 9, 3, p, 1, 3, p, 3, p, 3, 0, z, z, 1, 0, z, M, C, K3, C2, z)
    if entry == "fq_block_tail_proj_i8":
        N, H, W, C, K3, C2, CP, sp = a
        return L.fq_block_tail_proj_i8(p, p, p, 9, 3, p, p, p, 9, 3, sp, (H - 1) * sp + 1, (W - 1) * sp + 1, p, 3, p, 3, 0, z, z, 1, 0, z,
                                       N, H, W, C, K3, C2, CP, z)
    raise AssertionError("no caller for " + entry)


@pytest.mark.parametrize("row", T.REFUSALS, ids=[r.id for r in T.REFUSALS])
def test_the_first_refused_value_of_every_guard_is_refused(L, buf, row):
    assert row.value >= row.limit, "the table's own arithmetic: this row is not a refusal"
    if not row.exact and not row.id.endswith("_step"):
        assert row.value - row.limit < T.REACH[row.id], "not the smallest value the entry point's other rules let a call reach"
    rc = _call(L, buf, row.entry, row.args)
    assert rc == UNSUPPORTED, "%s%s: %s = %d (first refused: %d, %s) returned %d (%s)" % (
        row.entry, row.args, row.quantity, row.value, row.limit, row.guard, rc, L.fq_status_string(rc).decode())
    assert buf[2].raw == b"\0" * len(buf[2].raw)                        # nothing was written


def test_the_table_is_consistent_with_the_sources():
    """Every guard the table names exists (file and function), every product guard has a row one step above its first refusal,
    and the constants the table restates are the sources'."""
    csrc = os.path.join(ROOT, "pytorch-quantity_amd", "csrc")
    for g in {r.guard for r in T.REFUSALS} | {c.guard for c in T.GPU_CASES} | {s[0] for s in T.SHADOWED}:
        fname, func = g.split(": ")
        src = open(os.path.join(csrc, fname)).read()
        for f in func.split(" / "):
            assert re.search(r"\b%s\b" % re.escape(f), src), g
    ids = {r.id for r in T.REFUSALS}
    assert len(ids) == len(T.REFUSALS)
    for stem in ("c1_out", "c1_in", "c1_w", "sb_w", "c1add_out", "stem_out", "dwf_in", "gf_out", "bias_absmax", "bias_hist", "i8_kpq"):
        assert stem in ids and stem + "_step" in ids, stem
    common = open(os.path.join(csrc, "fq_common.h")).read()
    cus = int(re.search(r"constexpr int kCUs = (\d+);", common).group(1))
    assert T.POOL_STRIDE == cus * 64 * 256                              # (what the guard does with it: the max-pool test below)
    assert all(e in T.ARGS for e in {r.entry for r in T.REFUSALS})


def test_a_max_pool_whose_grid_stride_loop_would_wrap_is_refused(L, buf):
    """maxpool2d_f32_kernel walks `for (unsigned o = ...; o < total; o += stride)` with a stride of up to 2^22 outputs: from an
    index within one stride of 2^32 the addition wraps and the loop starts over, for ever.  The host refuses every `total` above
    2^32 - 1 - stride; the last admitted one leaves `o + stride` representable for every o < total."""
    stride = T.POOL_STRIDE
    last_admitted = (1 << 32) - 1 - stride
    assert (last_admitted - 1) + stride < 1 << 32                       # the largest index plus one stride still fits 32 bits
    first = last_admitted + 1
    assert first == 65472 * 256 * 256 == (1 << 32) - stride
    for planes in (65472, 65473, 65535, 65536):                         # 2^32 - 2^22 ... 2^32 outputs, kernel 1 / stride 1: the generic kernel
        assert planes * 256 * 256 >= first
        assert L.fq_maxpool2d_f32(buf[0], buf[0], planes, 256, 256, 1, 1, 1, 1, 0, 0, None) == UNSUPPORTED
    # ... and in the quad form of the 3x3 / 2 / 1 pool, whose input would pass 2^32 elements long before its outputs do
    assert L.fq_maxpool2d_f32(buf[0], buf[0], 16384, 512, 512, 3, 3, 2, 2, 1, 1, None) == UNSUPPORTED
    # a single plane of 2^31 elements: rows are addressed as `iy * W + ix` in an int
    assert L.fq_maxpool2d_f32(buf[0], buf[0], 1, 65536, 32768, 2, 2, 2, 2, 0, 0, None) == UNSUPPORTED


def test_the_host_predicates_answer_on_both_sides_of_their_limits(L):
    """The *_supported predicates launch nothing, so the last admitted value can be asked as well."""
    ok = L.fq_conv3x3_wino_f32_supported
    assert ok(127, 8, 64, 64, 1024) == 1 and ok(128, 8, 64, 64, 1024) == 0            # output bytes 2^31 - 2^24 / 2^31
    assert ok(127, 1024, 64, 64, 64) == 1 and ok(128, 1024, 64, 64, 64) == 0          # input bytes
    assert ok(1, 4096, 2, 2, 8128) == 1 and ok(1, 4096, 2, 2, 8192) == 0              # transformed weights: Cin * Cout * 64 bytes
    sb = L.fq_conv1x1_sb_supported
    assert 32768 * 21844 * 6 <= 0xffffffff < 32768 * 21848 * 6
    assert sb(32768, 21844) == 1 and sb(32768, 21848) == 0                            # the 6-byte pack ends below 4 GiB / does not
    assert sb(128, 256) == 1


# ---- the table's GPU rows, held to the same numbers -------------------------------------------------------------------------

def test_every_gpu_row_sits_where_the_table_says():
    assert len({c.id for c in T.GPU_CASES}) == len(T.GPU_CASES)
    for c in T.GPU_CASES:
        assert c.peak_bytes <= 26 * T.GiB, c.id
        assert c.kind in ("top", "bit31")
        if c.kind == "top":
            assert c.limit is not None and 0.98 * c.limit <= c.value < c.limit, c.id
            assert c.ragged or c.id in T.WORKLOAD_ROWS, c.id + ": a top row names its ragged dimensions"
            for name, v, tile in c.ragged:
                assert v % tile != 0, "%s: %s = %d is a multiple of %d" % (c.id, name, v, tile)
        else:
            assert c.big_bytes > 1 << 31, c.id
            if c.limit is not None:
                assert c.value < c.limit, c.id
        assert c.big_bytes < c.peak_bytes
    top = {c.id: c for c in T.GPU_CASES}
    n, cin, h, w, cout, _s = top["c1_top"].args
    assert (n * h * w) % 128 and cout % 128 and (n * h * w, cout) == (1032129, 1036)
    assert top["c1_top_ktail"].args[1] % 16 and top["c1_top_ktail"].args[1] % 8
    # the flat rows end in a scalar tail behind the 16-byte vectors
    assert T.N_FLAT % 4 == 3 and T.N_FLAT > 1 << 31
    # the bias rows: one with 16-byte planes, one with odd planes, both just above 2^31 elements
    assert top["bias_absmax_vec"].args[2] % 4 == 0 and top["bias_absmax_odd"].args[2] % 2 == 1
    for k in ("bias_absmax_vec", "bias_absmax_odd", "bias_hist_vec", "bias_hist_odd"):
        assert 1 << 31 < top[k].value < (1 << 31) * 1.001
    # the max-pool rows take the quad and the generic kernel, and stay clear of the refused range
    for k in ("pool_quad", "pool_generic"):
        planes, H, W, kh, kw, sh, sw, ph, pw = top[k].args
        Ho, Wo = T.out_size(H, kh, sh, ph), T.out_size(W, kw, sw, pw)
        quad = (kh, kw, sh, sw, ph, pw) == (3, 3, 2, 2, 1, 1) and W % 8 == 0 and Wo % 4 == 0 and Wo * 2 == W
        assert quad == (k == "pool_quad")
        assert planes * H * W > 1 << 31 and planes * Ho * Wo + T.POOL_STRIDE <= 0xffffffff and H * W <= 0x7fffffff
    # the banded int8 max-pool needs Q * Cpad / 16 <= 256 lanes
    _N, H, W, C = top["maxpool_i8_banded"].args[:4]
    assert T.out_size(W, 3, 2, 1) * (C // 16) <= 256 and 2 * (T.out_size(H, 3, 2, 1) - 1) < H
    _N, H, W, C = top["maxpool_i8_generic"].args[:4]
    assert top["maxpool_i8_generic"].args[4:6] == (2, 2)


@pytest.mark.parametrize("cid", sorted(T.WALKER_ROWS))
def test_the_geometry_walker_passes_the_top_row(cid, tmp_path):
    """Where a kernel's address arithmetic lives in a host-compilable header, its walker visits the first and the last pixels of
    the top row -- the lanes, strides and 32-bit indices of the real launch -- and exits non-zero on a load outside a source, a
    chunk written twice or not at all, or 32-bit pixel arithmetic that would wrap."""
    import subprocess
    src, args = T.WALKER_ROWS[cid]
    case = {c.id: c for c in T.GPU_CASES}[cid]
    tokens = args[-1].replace("/", ",").split(",")
    assert str(case.args[0]) in tokens and tokens.count("127") + tokens.count("254") >= 2      # the row's own batch and plane
    exe = str(tmp_path / src[:-4])
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", src)])
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0 and "ok, " in out.stdout, out.stdout + out.stderr
    if cid.startswith("cat"):
        assert "straddle 1" in out.stdout, out.stdout                   # the general family: a chunk put together from two sources


# ---- _float_conv.kind() repeats the float limits in Python -------------------------------------------------------------------

class FakeCuda(torch.Tensor):
    """A tensor that claims to be on the GPU: kind() reads attributes only (tests/test_grouped_f32_cpu.py)."""
    is_cuda = True


def _x(*shape):
    return torch.empty(*shape, device="meta").as_subclass(FakeCuda)     # no storage: the shapes below are gigabytes


# ResNet-101 at 512 x 512 (golden G13): (Cin, Cout, kernel, stride, padding, input plane) of the stem and of layer 1 / the head of layer 2
R101_512 = [(3, 64, 7, 2, 3, 512), (64, 64, 1, 1, 0, 128), (64, 64, 3, 1, 1, 128), (64, 256, 1, 1, 0, 128), (256, 64, 1, 1, 0, 128),
            (256, 128, 1, 1, 0, 128), (128, 128, 3, 2, 1, 128), (256, 512, 1, 2, 0, 128), (128, 512, 1, 1, 0, 64)]


def _c_admits(n, cin, cout, k, stride, pad, plane):
    out = T.out_size(plane, k, stride, pad)
    return n * cin * plane * plane < 1 << 30 and n * cout * out * out < 1 << 30 and k * k * cin * cout < 1 << 30


@pytest.mark.parametrize("batch", [255, 256])
def test_kind_chooses_an_own_kernel_exactly_where_the_c_guard_admits(L, buf, batch, monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.delenv("FQ_OWN_CONV1X1", raising=False)
    decided = set()
    for cin, cout, k, stride, pad, plane in R101_512:
        m = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=pad)
        admitted = _c_admits(batch, cin, cout, k, stride, pad, plane)
        got = _float_conv.kind(m, _x(batch, cin, plane, plane))
        assert (got is not None) == admitted, (batch, cin, cout, k, stride, plane, got)
        decided.add(admitted)
        if not admitted:                                                # ... and the C entry point of that layer says the same
            if k == 7:
                rc = _call(L, buf, "fq_conv_stem_f32", (batch, cin, plane, plane, cout, 7, 7, stride, pad))
            elif k == 1:
                rc = _call(L, buf, "fq_conv1x1_f32", (batch, cin, plane, plane, cout, stride))
            else:
                rc = _call(L, buf, "fq_conv_kxk_f32", (batch, cin, plane, plane, cout, k, k, stride, pad))
            assert rc == UNSUPPORTED, (batch, cin, cout, k)
    assert decided == ({True} if batch == 255 else {True, False})
    if batch == 256:                                                    # 16 MiB per image: exactly 2^30 elements at 256 images
        assert not _c_admits(256, 3, 64, 7, 2, 3, 512) and not _c_admits(256, 64, 256, 1, 1, 0, 128) and _c_admits(256, 128, 512, 1, 1, 0, 64)


def test_kind_agrees_with_the_c_guards_of_the_depthwise_and_grouped_kernels(L, buf):
    """"dw" and "g" at the same limits: 2^30 input or output elements, and for "g" 2^30 weights."""
    from common.quantity import _float_conv
    dw = torch.nn.Conv2d(64, 64, 3, padding=1, groups=64)
    assert _float_conv.kind(dw, _x(255, 64, 256, 256), depthwise=True) == "dw"
    assert _float_conv.kind(dw, _x(256, 64, 256, 256), depthwise=True) is None
    assert _call(L, buf, "fq_dwconv_f32", (256, 64, 256, 256, 3, 3, 1, 1)) == UNSUPPORTED
    wide = torch.nn.Conv2d(64, 64, 3, padding=2, groups=64)                # the output plane is larger than the input's
    assert _float_conv.kind(wide, _x(252, 64, 256, 256), depthwise=True) == "dw" and 252 * 64 * 258 * 258 < 1 << 30
    assert _float_conv.kind(wide, _x(253, 64, 256, 256), depthwise=True) is None
    assert _call(L, buf, "fq_dwconv_f32", (253, 64, 256, 256, 3, 3, 1, 2)) == UNSUPPORTED
    g = torch.nn.Conv2d(8, 64, 1, groups=2)
    assert _float_conv.kind(g, _x(255, 8, 256, 256), grouped=True) == "g"
    assert _float_conv.kind(g, _x(256, 8, 256, 256), grouped=True) is None       # 2^30 outputs
    assert _call(L, buf, "fq_gconv_f32", (256, 8, 256, 256, 64, 2, 1, 1, 1, 0)) == UNSUPPORTED
    x1 = _x(1, 29128 * 64, 1, 1)
    assert _float_conv.kind(torch.nn.Conv2d(29127 * 64, 29127 * 64, 3, padding=1, groups=29127, device="meta"), _x(1, 29127 * 64, 1, 1),
                            grouped=True) == "g"                                  # 2^30 - 4096 weights
    assert _float_conv.kind(torch.nn.Conv2d(29128 * 64, 29128 * 64, 3, padding=1, groups=29128, device="meta"), x1, grouped=True) is None
    assert _call(L, buf, "fq_gconv_f32", (1, 29128 * 64, 1, 1, 29128 * 64, 29128, 3, 3, 1, 1)) == UNSUPPORTED


def test_kind_and_the_linear_path_decline_a_matrix_of_2_30_weights(L, buf, monkeypatch):
    from common.quantity import _float_conv
    x = _x(1, 32768, 1, 1)
    assert _float_conv.kind(torch.nn.Conv2d(32768, 32764, 1, device="meta"), x) == "c1"          # 2^30 - 2^17 weights
    assert _float_conv.kind(torch.nn.Conv2d(32768, 32768, 1, device="meta"), x) is None
    assert _call(L, buf, "fq_conv1x1_f32", (1, 32768, 1, 1, 32768, 1)) == UNSUPPORTED
    lin = torch.nn.Linear(32768, 32768, device="meta")
    assert lin.in_features * lin.out_features == 1 << 30
    x2 = torch.empty(4, 32768, device="meta").as_subclass(FakeCuda)
    calls = []
    monkeypatch.setattr(_float_conv._native, "conv1x1_f32", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("launched")))
    with torch.no_grad():
        assert _float_conv.call_linear_qd(lin, x2, 4, 8) is None
    assert calls == [] and not _float_conv.is_off(lin) and "wt_linear" not in _float_conv.state(lin)     # declined by the guard itself
    # the split-bf16 form stops earlier: its pack holds 6 bytes per weight behind 32-bit byte offsets
    from common.quantity import _native
    assert _native.conv_sb_supported(32768, 21844) and not _native.conv_sb_supported(32768, 21848)
