"""The resident NewAdd (add_resident_16_regs, csrc/fq_resident.h) in every kernel it is inlined into, over whole operand domains
and on both sides of every boundary of its form selection, against the exact integer rule of tests/add_rule.py -- which
tests/test_add_rule_cpu.py ties to the CPU oracle's fp32 chain.  No expected value below comes from a kernel; every comparison
is torch.equal.

  * fq_add_resident: all 65 536 pairs of two int8 operands; an int16 operand's 65 536 values against 16 boundary values of the
    other, in either role and for either type of the other; one launch per parameter set of tests/add_form_cases.py.
  * the fused entry points, driven through a PASS-THROUGH convolution: weights 2 I, shift 1 and a zero bias give
    (2 x + 1 + sign) >> 1 = x for every int8 x, so the convolution's result operand -- unpacked by code of its own in every
    kernel -- takes every value at every lane against every value of the shortcut.
  * which form ran is fq_add_resident_form's answer (_native.add_resident_form); the coverage tests assert that every form is
    reached with every operand type it can take, ReLU on and off, through every entry point.

A mismatch is reported as the operands of the first differing element.   pytest -m gpu"""
import numpy as np
import pytest
import torch

import add_form_cases as ac
from add_rule import add_rule

pytestmark = pytest.mark.gpu

V8 = (-128, -127, -65, -64, -63, -2, -1, 0, 1, 2, 63, 64, 65, 100, 126, 127)
V16 = (-32768, -32767, -16384, -129, -128, -65, -64, -1, 0, 1, 64, 127, 128, 16384, 32766, 32767)
DT = {1: torch.int8, 2: torch.int16}
SENTINEL8, SENTINEL16 = 0x5A, 0x5A5A


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available()
    from common.quantity import _native
    _native.lib()
    return _native


def _idx(n):
    return torch.arange(n, dtype=torch.int64, device="cuda")


def _full(i, nbytes):
    """every value of the type, by the low bits of the index"""
    return (i & 0xff) - 128 if nbytes == 1 else (i & 0xffff) - 32768


def _pick(values, j):
    return torch.tensor(values, dtype=torch.int64, device="cuda")[j]


def _pairs(xb, yb):
    """[(x, y)] int64 index arithmetic -> typed flat tensors: the operand layouts of fq_add_resident's tests.  Two int8 operands:
    x = (i & 255) - 128, y = (i >> 8) - 128 over 65 536 elements.  With an int16 operand: it runs through all its values by
    i & 0xffff while the other takes one of 16 boundary values by i >> 16 (1 M elements); two int16 operands in both roles."""
    if (xb, yb) == (1, 1):
        i = _idx(1 << 16)
        return [((i & 255) - 128, (i >> 8) - 128)]
    i = _idx(1 << 20)
    out = []
    if yb == 2:
        out.append((_pick(V8 if xb == 1 else V16, i >> 16), _full(i, 2)))
    if xb == 2:
        out.append((_full(i, 2), _pick(V8 if yb == 1 else V16, i >> 16)))
    return out


@pytest.fixture(scope="module")
def operands():
    """{(x_bytes, y_bytes): [(x, y)]} as [1, H, W, 64] device tensors, built once and never written."""
    out = {}
    for (xb, yb) in ac.TYPE_PAIRS:
        out[(xb, yb)] = [(x.to(DT[xb]).view(1, -1, 32 if x.numel() == 1 << 16 else 128, 64), y.to(DT[yb]).view(1, -1, 32 if y.numel() == 1 << 16 else 128, 64))
                         for x, y in _pairs(xb, yb)]
    return out


def _pair_count(x, y):
    return int(torch.unique((x.flatten().to(torch.int64) + 32768) * 65536 + y.flatten().to(torch.int64) + 32768).numel())


def _same(got, want, x, y, what):
    assert (got is None) == (want is None), what
    if got is None or torch.equal(got, want):
        return
    bad = (got != want).flatten()
    i = int(bad.nonzero()[0])
    raise AssertionError("%s: %d of %d differ; first at element %d: x = %d, y = %d, got %d, want %d" % (
        what, int(bad.sum()), bad.numel(), i, int(x.flatten()[i]), int(y.flatten()[i]), int(got.flatten()[i]), int(want.flatten()[i])))


def _expect(x, y, gx, gy, ib, relu):
    g = max(0, gx, gy)
    return add_rule(x, y, gx, gy, ib, bool(relu), g if g <= 8 else None)


# ---------------------------------------------------------------- fq_add_resident
def test_the_operand_tensors_hold_the_domains_they_claim(operands):
    (x, y), = operands[(1, 1)]
    assert x.dtype == y.dtype == torch.int8 and tuple(x.shape) == (1, 32, 32, 64) and _pair_count(x, y) == 1 << 16
    for (xb, yb), n in (((1, 2), 1), ((2, 1), 1), ((2, 2), 2)):
        assert len(operands[(xb, yb)]) == n
        for x, y in operands[(xb, yb)]:
            assert x.dtype == DT[xb] and y.dtype == DT[yb] and x.numel() == 1 << 20 and _pair_count(x, y) == 16 << 16
    for vals, lim in ((V8, 128), (V16, 32768)):
        assert len(set(vals)) == 16 and {-lim, 1 - lim, -1, 0, 1, lim - 2, lim - 1, -64, 64} <= set(vals)


def test_the_case_list_covers_what_it_claims(nat):
    """Conditions, not measurements: each form with every operand-type pair it can take and with ReLU on and off, both sides of
    every edge of the selection and of the ABI's ranges, and the project's own parameter sets."""
    cov = ac.coverage(nat.add_resident_form)
    assert cov["forms"] == {(f, xb, yb, relu) for (xb, yb) in ac.TYPE_PAIRS for f in ac.reachable_forms(xb, yb) for relu in (0, 1)}
    assert {f for f, xb, yb, relu in cov["forms"] if xb == 1} == {0, 1, 2, 3} and {f for f, xb, yb, relu in cov["forms"] if xb == 2} == {0, 1, 2}
    assert cov["edges"] == {(n, v) for n, vs in ac.EDGES.items() for v in vs}
    assert set(ac.project_sets()) <= set(ac.triples())


def _refused_untouched(nat, x, y, gx, gy, ib, relu):
    """a wide output at g > 8: FQ_ERR_UNSUPPORTED, and neither output written"""
    wide = torch.full(x.shape, SENTINEL16, dtype=torch.int16, device="cuda")
    narrow = torch.full(x.shape, SENTINEL8, dtype=torch.int8, device="cuda")
    rc = nat.lib().fq_add_resident(x.data_ptr(), x.element_size(), gx, y.data_ptr(), y.element_size(), gy, wide.data_ptr(), max(0, gx, gy),
                                   narrow.data_ptr(), ib, relu, x.numel(), nat._stream(x))
    torch.cuda.synchronize()
    assert rc == -4 and bool((wide == SENTINEL16).all()) and bool((narrow == SENTINEL8).all()), (gx, gy, ib, rc)


@pytest.mark.parametrize("pair", ac.TYPE_PAIRS, ids=lambda p: "x%d_y%d" % p)
def test_add_resident_is_the_rule_over_whole_operand_domains(nat, operands, pair):
    xb, yb = pair
    forms, refused = set(), 0
    for n, (gx, gy, ib) in enumerate(ac.triples()):
        g = max(0, gx, gy)
        for relu in (0, 1):
            forms.add((nat.add_resident_form(xb, gx, yb, gy, ib, relu), relu))
            for x, y in operands[pair]:
                what = "x_bytes %d y_bytes %d gx %d gy %d ib %d relu %d" % (xb, yb, gx, gy, ib, relu)
                want_w, want_n = _expect(x, y, gx, gy, ib, relu)
                if g > 8:
                    assert want_w is None
                    _, narrow = nat.add_resident(x, gx, y, gy, False, 0, True, ib, relu)
                    _same(narrow, want_n, x, y, what + " narrow (alone: no wide sum at g > 8)")
                    if relu == 0 and x is operands[pair][0][0]:
                        _refused_untouched(nat, x, y, gx, gy, ib, relu)
                        refused += 1
                    continue
                wide, narrow = nat.add_resident(x, gx, y, gy, True, g, True, ib, relu)
                _same(wide, want_w, x, y, what + " wide")
                _same(narrow, want_n, x, y, what + " narrow")
                if n % 10 == 0:
                    wide, none = nat.add_resident(x, gx, y, gy, True, g, False, ib, relu)
                    assert none is None
                    _same(wide, want_w, x, y, what + " wide alone")
                    none, narrow = nat.add_resident(x, gx, y, gy, False, 0, True, ib, relu)
                    assert none is None
                    _same(narrow, want_n, x, y, what + " narrow alone")
    assert forms == {(f, relu) for f in ac.reachable_forms(xb, yb) for relu in (0, 1)} and refused >= 4


# ---------------------------------------------------------------- the fused entry points behind a pass-through convolution
def _passthrough(nat, C, K, R):
    """int8 [K][R][R][C] weights with 2 at (k, centre, centre, k mod C), a zero bias; with shift 1 the tail returns its input."""
    w = torch.zeros(K, C, R, R, device="cuda")
    w[torch.arange(K), torch.arange(K) % C, R // 2, R // 2] = 2.0
    return nat.pack_weight_krsc(w), torch.zeros(K, device="cuda")


def _fused_operands(yb, width):
    """(x', y) as the [M][width] tensors a fused kernel adds (x' the convolution's result), in the layouts of _pairs."""
    x, y = _pairs(1, yb)[0]
    return x.to(torch.int8).view(1, -1, 16, width), y.to(DT[yb]).view(1, -1, 16, width)


def _stacked_operands(yb):
    """The same for a 64 -> 128 convolution whose weights are the identity stacked twice: output channel k reads input channel
    k mod 64, so x'[m][k] = x'[m][k + 64] and the pairs are laid out by t = 64 m + k mod 64 and the half h = k >> 6.  int8
    shortcut: x' = (t & 255) - 128, y = ((t >> 8) | (h << 7)) - 128 over 512 pixels.  int16 shortcut: as _pairs (x' changes only
    every 65 536 elements).  Returns (x [M][64], x' [M][128], y [M][128])."""
    if yb == 1:
        j = _idx(1 << 16)
        m, k = j >> 7, j & 127
        t = m * 64 + (k & 63)
        xo, y = (t & 255) - 128, ((t >> 8) | ((k >> 6) << 7)) - 128
    else:
        xo, y = _pairs(1, 2)[0]
    xo = xo.to(torch.int8).view(1, -1, 16, 128)
    assert torch.equal(xo[..., :64], xo[..., 64:])
    return xo[..., :64].contiguous(), xo, y.to(DT[yb]).view(1, -1, 16, 128)


def build_fused(nat):
    """Everything the fused tests share: parameter sets, operands, pass-through weights (also built by the child process of the
    streaming-kernel test, tests/add_forms_stream_child.py)."""
    f = {"sets": ac.fused_sets(nat.add_resident_form)}
    for yb in (1, 2):
        f[("flat64", yb)] = _fused_operands(yb, 64)
        f[("flat128", yb)] = _fused_operands(yb, 128)
        f[("stacked", yb)] = _stacked_operands(yb)
    for name, (C, K, R) in (("w1x1_64", (64, 64, 1)), ("w3x3_64", (64, 64, 3)), ("w3x3_128", (128, 128, 3)), ("w128", (128, 128, 1)),
                            ("wstack", (64, 128, 1))):
        f[name] = _passthrough(nat, C, K, R)
    return f


@pytest.fixture(scope="module")
def fused(nat):
    """build_fused, once per module"""
    return build_fused(nat)


def test_the_fused_sets_cover_every_class(nat, fused):
    form = nat.add_resident_form
    classes = {(form(1, gx, yb, gy, ib, relu), yb, relu) for (gx, gy, ib, yb, relu) in fused["sets"]}
    assert classes == {(f, yb, relu) for f in ac.FORMS for yb in (1, 2) for relu in (0, 1)}
    assert {(ac.quantities(gx, gy, ib)["shy"], relu) for (gx, gy, ib, yb, relu) in fused["sets"] if yb == 2} >= {(0, 0), (0, 1), (1, 0), (1, 1)}
    for yb in (1, 2):
        for key, pairs in (("flat64", 1), ("flat128", 1), ("stacked", 1)):
            ops = fused[(key, yb)]
            assert _pair_count(ops[-2], ops[-1]) == (1 << 16 if yb == 1 else 16 << 16)


def _logged(nat, fn):
    nat.conv_variant_log = log = {}
    try:
        out = fn()
    finally:
        nat.conv_variant_log = None
    assert len(log) == 1 and sum(log.values()) == 1, log
    return out, next(iter(log))


def _check_fused(call, sets, xo, y_of, label):
    """call(gx, gy, ib, relu, y, want_wide, g) -> (wide, narrow) for every parameter set, against the rule on (x', y)."""
    ran = 0
    for (gx, gy, ib, yb, relu) in sets:
        y = y_of(yb)
        g = max(0, gx, gy)
        want_w, want_n = _expect(xo, y, gx, gy, ib, relu)
        wide, narrow = call(gx, gy, ib, relu, y, g <= 8, g)
        what = "%s: ob %d g_res %d ib %d relu %d res_bytes %d" % (label, gx, gy, ib, relu, yb)
        _same(wide, want_w, xo, y, what + " wide")
        _same(narrow, want_n, xo, y, what + " narrow")
        ran += 1
    return ran


# (R, C, K) -> (operands, weights) of `fused`, and the kernels the selector may send the layer to WITH a fused residual, by default and
# where the opt-in streaming 1x1 kernel is on (csrc/fq_conv1x1_i8.hip; it declines per-channel shifts, which fall back)
CONV_LAYERS = {(1, 64, 64): ("flat64", "w1x1_64"), (3, 64, 64): ("flat64", "w3x3_64"), (3, 128, 128): ("flat128", "w3x3_128"),
               (1, 128, 128): ("flat128", "w128"), (1, 64, 128): ("stacked", "wstack")}
DEFAULT_KERNELS = {(1, 64, 64): {"tile_c64"}, (3, 64, 64): {"tile_c64"}, (3, 128, 128): {"dma2", "dma3"}, (1, 128, 128): {"tile_c128"},
                   (1, 64, 128): {"tile_c64"}}
STREAM_LAYERS = ((1, 64, 64), (1, 64, 128), (1, 128, 128))


def conv_add_layers(nat, fused, pcs, layers):
    """fq_conv2d_i8_add_resident (pcs: its _pcs sibling with the constant shift vector) behind the pass-through convolution of every
    layer, both residual types, every parameter set of fused["sets"], against the rule; the pass-through is asserted on
    fq_conv2d_i8_resident's output first: a comparison with the input tensor.  Returns {layer: kernel names the add launches ran}."""
    names = {}
    for (R, C, K) in layers:
        rs = nat.ShiftVec(torch.ones(K, dtype=torch.int32, device="cuda"), 1, 1) if pcs else 1
        opkey, wkey = CONV_LAYERS[(R, C, K)]
        w, b = fused[wkey]
        pad = (R // 2, R // 2)
        variants = set()
        for yb in (1, 2):
            ops = fused[(opkey, yb)]
            x, xo, y_all = ops[0], ops[-2], ops[-1]
            (_, q), v = _logged(nat, lambda: nat.conv2d_i8_resident(x, w, b, (1, 1), pad, (1, 1), rs, 0, False, True, False))
            assert torch.equal(q, xo), "the %dx%d convolution %d -> %d is not a pass-through" % (R, R, C, K)

            def call(gx, gy, ib, relu, y, want_wide, g):
                out, v = _logged(nat, lambda: nat.conv2d_i8_add_resident(x, w, b, (1, 1), pad, (1, 1), rs, gx, y, gy, want_wide, g, True, ib, relu))
                variants.add(v.split("/")[0])
                return out

            sets = [s for s in fused["sets"] if s[3] == yb]
            label = "conv %dx%d %d -> %d + add%s" % (R, R, C, K, " (pcs)" if pcs else "")
            assert _check_fused(call, sets, xo, lambda b_: y_all, label) == len(sets)
        names[(R, C, K)] = variants
    return names


@pytest.mark.parametrize("pcs", [False, True], ids=["per_tensor", "pcs"])
def test_conv_add_resident_is_the_rule_behind_a_pass_through_convolution(nat, fused, pcs):
    """Five layers: a 1x1 identity with C = K = 64, a 3x3 one (centre tap, padding 1) of the same width, a 3x3 and a 1x1 one at 128
    channels, and 64 -> 128 with the identity stacked twice.  With a fused residual the selector keeps both 64-channel layers on
    the tile kernel's 64-channel path (a 3x3 layer does NOT leave it: asserted, so that a change of the selector is noticed),
    takes the 128-channel 1x1 layer on its whole-line path, and sends the deep 3x3 reduction at 128 channels to the LDS-DMA kernel,
    whose epilogue unpacks the convolution's result from its own staging."""
    names = conv_add_layers(nat, fused, pcs, sorted(CONV_LAYERS))
    for layer, allowed in DEFAULT_KERNELS.items():
        assert names[layer] and names[layer] <= allowed, (layer, names[layer])
    assert names[(3, 64, 64)] == names[(1, 64, 64)] and not (names[(1, 64, 64)] & names[(3, 128, 128)])


def test_the_streaming_1x1_kernel_s_add_epilogue_is_the_rule():
    """csrc/fq_conv1x1_i8.hip unpacks the convolution's result from registers and reads the shortcut by buffer loads: its add
    epilogue is a site of its own.  The kernel is opt-in (FQ_CONV_STREAM=1, read once per process), hence a fresh child process:
    tests/add_forms_stream_child.py runs the 1x1 pass-through layers there (64 -> 64, 64 -> 128, 128 -> 128: its three tile shapes)
    over the same parameter sets and operands, against the rule, and asserts that the log shows `stream` for the per-tensor entry
    and the default kernels for the _pcs entry, which the streaming kernel declines."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "add_forms_stream_child.py")],
                       env=dict(os.environ, FQ_CONV_STREAM="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "add_forms_stream_child: OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "per_tensor stream stream stream" in r.stdout and "pcs tile_c64 tile_c64 tile_c128" in r.stdout, r.stdout[-1000:]


@pytest.mark.parametrize("shape", ["128to128", "64to128_stacked"])
def test_block_tail_is_the_rule_behind_a_pass_through_conv3(nat, fused, shape):
    """fq_block_tail_i8 without a next conv1: C = K3 = 128 with the identity, and C = 64 -> K3 = 128 with the identity stacked
    twice (output channel k reads x[k mod 64])."""
    w3, b3 = fused["w128" if shape == "128to128" else "wstack"]
    C = 128 if shape == "128to128" else 64

    def ops(yb):
        o = fused[("flat128" if shape == "128to128" else "stacked", yb)]
        return (o[0], o[0], o[1]) if shape == "128to128" else o

    def call(gx, gy, ib, relu, y, want_wide, g):
        x = ops(y.element_size())[0]
        assert nat.block_tail_supported(C, 128, 0, 1, 0, gx, gy, y.element_size(), ib)
        (wide, narrow, q1), v = _logged(nat, lambda: nat.block_tail_i8(x, w3, b3, 1, gx, y, gy, want_wide, g, True, ib, relu))
        assert v == "block_tail/128" and q1 is None
        return wide, narrow

    ran = 0
    for yb in (1, 2):
        x, xo, y = ops(yb)
        _, q = nat.conv2d_i8_resident(x, w3, b3, (1, 1), (0, 0), (1, 1), 1, 0, False, True, False)
        assert torch.equal(q, xo), "conv3 is not a pass-through"
        ran += _check_fused(call, [s for s in fused["sets"] if s[3] == yb], xo, lambda b_: ops(b_)[2], "block tail " + shape)
    assert ran == len(fused["sets"])


def test_block_tail_with_the_next_conv1_reads_the_rule_s_narrow_output(nat, fused, oracle):
    """One case with the fused next conv1 (128 -> 64, random weights): q1 is the oracle's integer convolution and tail applied to
    the RULE's narrow output, wide and narrow are the rule's."""
    from int_conv_ref import conv2d_int_fast
    gx, gy, ib, relu, rs1 = 4, 5, 4, 1, 10
    assert nat.add_resident_form(1, gx, 2, gy, ib, relu) == 3
    w3, b3 = fused["w128"]
    xo, y = fused[("flat128", 2)]
    M = 1024                                                              # the first 1024 pixels: x' = -128 and -127 against every y
    xo, y = xo.view(-1, 128)[:M].view(1, 32, 32, 128).contiguous(), y.view(-1, 128)[:M].view(1, 32, 32, 128).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(5)
    w1f = torch.randint(-127, 128, (64, 128, 1, 1), device="cuda", generator=gen).float()
    b1 = torch.randint(-100, 101, (64,), device="cuda", generator=gen).float()
    wide, narrow, q1 = nat.block_tail_i8(xo, w3, b3, 1, gx, y, gy, True, 5, True, ib, relu, nat.pack_weight_krsc(w1f), b1, rs1, True)
    want_w, want_n = _expect(xo, y, gx, gy, ib, relu)
    _same(wide, want_w, xo, y, "block tail + conv1 wide")
    _same(narrow, want_n, xo, y, "block tail + conv1 narrow")
    acc = conv2d_int_fast(want_n.cpu().numpy().astype(np.int32).transpose(0, 3, 1, 2), w1f.cpu().numpy().astype(np.int32))
    t1 = np.maximum(oracle.recon_epilogue(acc.astype(np.float32), b1.cpu().numpy(), rs1, 0, 8), 0)
    assert np.array_equal(q1.cpu().numpy().astype(np.float32), t1.transpose(0, 2, 3, 1)) and int((q1 != 0).sum()) > 0


def test_block_tail_proj_is_the_rule_behind_two_pass_through_convolutions(nat, fused):
    """fq_block_tail_proj_i8, C = CP = 64 -> K3 = 128 with stacked identities for conv3 AND the projection: the block's input is
    one operand, the projection's input the other (an int8 shortcut on the grid obp): t = 64 m + c, x = (t & 255) - 128,
    xp = (t >> 8) - 128 over 1024 pixels, every pair in both halves of the 128 channels."""
    w3, b3 = fused["wstack"]
    t = _idx(1 << 16)
    x = ((t & 255) - 128).to(torch.int8).view(1, 32, 32, 64)
    xp = ((t >> 8) - 128).to(torch.int8).view(1, 32, 32, 64)
    xo, yo = torch.cat([x, x], dim=3), torch.cat([xp, xp], dim=3)
    assert _pair_count(xo, yo) == 1 << 16
    _, q = nat.conv2d_i8_resident(xp, w3, b3, (1, 1), (0, 0), (1, 1), 1, 0, False, True, False)
    assert torch.equal(q, yo), "the projection is not a pass-through"

    def call(gx, gy, ib, relu, y, want_wide, g):
        assert nat.block_tail_proj_supported(64, 128, 0, 64, 1, 0, 1, 1)
        (wide, narrow, q1), v = _logged(nat, lambda: nat.block_tail_proj_i8(x, w3, b3, 1, gx, xp, w3, b3, 1, gy, 1, want_wide, g, True, ib, relu))
        assert v == "block_tail_proj/128" and q1 is None
        return wide, narrow

    sets = [s for s in fused["sets"] if s[3] == 1]
    assert _check_fused(call, sets, xo, lambda b_: yo, "block tail proj") == len(sets)
    assert {nat.add_resident_form(1, s[0], 1, s[1], s[2], s[4]) for s in sets} == {0, 1, 2, 3}


def _add_up_operands(xb, yb):
    """[(x [1][H][W][64], y [1][H / 2][W / 2][64])]: coarse element u = (h2 * W2 + w2) * 64 + c meets its four fine elements
    d = 2 (h & 1) + (w & 1).  Two int8 operands: y = (u & 255) - 128 and x = 4 (u >> 8) + d - 128 (16 384 coarse elements).  An
    int16 y through all its values: y = (u & 0xffff) - 32768, x = V[4 (u >> 16) + d]; an int16 x through all of them:
    y = V[u & 15], x = 4 (u >> 4) + d - 32768 (262 144 coarse elements each)."""
    def planes(W2):
        W = 2 * W2
        f = _idx(W * W * 64)
        h, w, c = f // (W * 64), (f // 64) % W, f & 63
        return _idx(W2 * W2 * 64), ((h >> 1) * W2 + (w >> 1)) * 64 + c, (h & 1) * 2 + (w & 1), W
    out = []
    if (xb, yb) == (1, 1):
        uc, u, d, W = planes(16)
        out.append((4 * (u >> 8) + d - 128, (uc & 255) - 128, W))
    else:
        uc, u, d, W = planes(64)
        if yb == 2:
            out.append((_pick(V8 if xb == 1 else V16, 4 * (u >> 16) + d), (uc & 0xffff) - 32768, W))
        if xb == 2:
            out.append((4 * (u >> 4) + d - 32768, _pick(V8 if yb == 1 else V16, uc & 15), W))
    return [(x.to(DT[xb]).view(1, W, W, 64), y.to(DT[yb]).view(1, W // 2, W // 2, 64)) for x, y, W in out]


@pytest.mark.parametrize("pair", ac.TYPE_PAIRS, ids=lambda p: "x%d_y%d" % p)
def test_add_up_resident_is_the_rule_on_the_repeated_coarse_operand(nat, pair):
    """fq_add_up_resident with up = 2, the coarse plane laid out so that every (x, y) pair of the domains above still occurs; one
    parameter set per (form, relu) class the operand types can reach."""
    xb, yb = pair
    sets = ac.class_sets(nat.add_resident_form, xb, yb)
    assert {(nat.add_resident_form(xb, s[0], yb, s[1], s[2], s[3]), s[3]) for s in sets} == {(f, r) for f in ac.reachable_forms(xb, yb) for r in (0, 1)}
    for x, y in _add_up_operands(xb, yb):
        yu = y.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        assert _pair_count(x, yu) == (1 << 16 if pair == (1, 1) else 16 << 16)
        assert nat.add_up_supported(2, x.shape[1], x.shape[2], 64)
        for (gx, gy, ib, relu) in sets:
            g = max(0, gx, gy)
            want_w, want_n = _expect(x, yu, gx, gy, ib, relu)
            wide, narrow = nat.add_up_resident(x, gx, y, gy, 2, g <= 8, g if g <= 8 else 0, True, ib, relu)
            what = "add_up x_bytes %d y_bytes %d gx %d gy %d ib %d relu %d" % (xb, yb, gx, gy, ib, relu)
            _same(wide, want_w, x, yu, what + " wide")
            _same(narrow, want_n, x, yu, what + " narrow")
