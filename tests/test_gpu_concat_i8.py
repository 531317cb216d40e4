"""Concatenation and nearest upsampling of resident int8 activations (fq_concat_i8_nhwc, csrc/fq_concat_i8.hip) against the index
rule in NumPy, and resident.enable(..., concat=True) on Fire / FPN style nets and calibrated models.  Everything is integers:
every comparison is exact.   pytest -m gpu"""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import cases
import concat_nets as cn
import depthwise_nets as dn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = -1, -4
SENTINEL, GUARD = 0x5A, 64


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _pad16(c):
    return (c + 15) // 16 * 16


# ---------------------------------------------------------------- 1. the kernel against the index rule
def _sources(rng, case):
    """int8 NHWC sources over the whole range (-128 and 127 included) whose padding channels hold non-zero garbage."""
    N, H, W, C0, C1, u0, u1 = case
    out = []
    for C, u in ((C0, u0), (C1, u1)):
        if C == 0:
            continue
        a = rng.integers(-128, 128, size=(N, H // u, W // u, _pad16(C))).astype(np.int8)
        a.flat[::7] = -128
        a.flat[3::11] = 127
        a[..., C:] = np.where(a[..., C:] == 0, 77, a[..., C:])
        out.append((a, C, u))
    return out


def _index_rule(case, srcs, relu):
    N, H, W = case[:3]
    total = sum(C for _a, C, _u in srcs)
    want = np.zeros((N, H, W, _pad16(total)), dtype=np.int8)
    hh, ww = np.arange(H), np.arange(W)
    base = 0
    for a, C, u in srcs:
        want[..., base:base + C] = a[:, hh // u][:, :, ww // u][..., :C]
        base += C
    return np.maximum(want, 0) if relu else want


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", cn.KERNEL_CASES, ids=lambda c: "n%d_%dx%d_c%d_%d_up%d_%d" % c)
def test_concat_kernel_vs_index_rule(nat, case, relu):
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    srcs = _sources(rng, case)
    want = _index_rule(case, srcs, relu)
    dev = [(torch.from_numpy(a).cuda(), C, u) for a, C, u in srcs]
    # the output is a view inside a larger buffer: sentinel bytes in front of and behind it must survive
    buf = torch.full((GUARD + want.size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
    view = buf[GUARD:GUARD + want.size].view(want.shape)
    assert view.data_ptr() % 16 == 0
    got = nat.concat_i8_nhwc(dev, relu, out=view)
    assert got is view
    host = buf.cpu().numpy()
    np.testing.assert_array_equal(host[GUARD:GUARD + want.size].reshape(want.shape), want)
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + want.size:] == SENTINEL).all()
    total = sum(C for _a, C, _u in srcs)
    assert not host[GUARD:GUARD + want.size].reshape(want.shape)[..., total:].any()        # the padding channels are zero
    own = nat.concat_i8_nhwc(dev, relu)                                                    # ... and the allocating form
    assert tuple(own.shape) == want.shape and own.shape[-1] == _pad16(total)
    np.testing.assert_array_equal(own.cpu().numpy(), want)
    for (a, _C, _u), (d, _c, _up) in zip(srcs, dev):
        np.testing.assert_array_equal(d.cpu().numpy(), a)                                   # the sources are only read


def test_the_case_list_covers_each_path_it_claims(tmp_path):
    """Through the host geometry header's own classification (cat_chunk_class, printed per case by scripts/concat_geom_check.cpp):
    one 16-byte load, aligned dwords, byte-shifted dwords, chunks that straddle C0 -- with and without an upsampled operand."""
    exe = str(tmp_path / "concat_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "concat_geom_check.cpp")])
    out = subprocess.run([exe, "maxsrc=2"] + [cn.case_arg(c) for c in cn.KERNEL_CASES], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    by_arg = {cn.case_arg(c): c for c in cn.KERNEL_CASES}
    rows = {}
    for line in out.stdout.splitlines():
        if line.startswith("case "):
            key, rest = line[5:].split(":")
            w = rest.split()
            rows[by_arg[key]] = dict(zip(w[0::2], (int(v) for v in w[1::2])))
    assert set(rows) == set(cn.KERNEL_CASES)
    plain = {c: r for c, r in rows.items() if c[5] == 1 and c[6] == 1}
    ups = {c: r for c, r in rows.items() if c[5] > 1 or c[6] > 1}
    for name, group in (("plain", plain), ("upsampled", ups)):
        for kind in ("aligned16", "dword", "byte", "straddle"):
            assert any(r[kind] for r in group.values()), (name, kind)
    # the cases named "aligned path" hold nothing else; C0 % 16 == 0 never needs the assembling path
    for c, r in rows.items():
        if c[3] % 16 == 0:
            assert r["dword"] == r["byte"] == r["straddle"] == 0, (c, r)
    assert rows[(3, 7, 9, 20, 44, 1, 1)]["dword"] and not rows[(3, 7, 9, 20, 44, 1, 1)]["byte"]
    assert rows[(1, 6, 6, 17, 30, 1, 1)]["byte"] and rows[(1, 6, 6, 17, 30, 1, 1)]["straddle"]
    assert {c[4] for c in cn.KERNEL_CASES} >= {0} and {c[5] for c in cn.KERNEL_CASES} == {1, 2, 4}
    assert any(c[3] + c[4] == 16 for c in cn.KERNEL_CASES) and any(_pad16(c[3] + c[4]) < _pad16(c[3]) + _pad16(c[4]) for c in cn.KERNEL_CASES)


# ---------------------------------------------------------------- 2. what the entry point declines
def _raw(nat, srcs, nsrc, out, cpad_out, relu, N, H, W):
    arr = (nat._CatSrc * max(len(srcs), 1))()
    for i, (q, C, cpad, up) in enumerate(srcs):
        arr[i].q, arr[i].C, arr[i].Cpad, arr[i].up = (q.data_ptr() if q is not None else None), C, cpad, up
    return nat.lib().fq_concat_i8_nhwc(arr, nsrc, ctypes.c_void_p(out.data_ptr()) if out is not None else None, cpad_out, relu, N, H, W, None)


def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any of these geometries, and nothing may be launched."""
    a = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    b = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    out = torch.full((1, 8, 8, 64), 5, dtype=torch.int8, device="cuda")
    ok2 = [(a, 16, 16, 1), (b, 16, 16, 1)]
    assert _raw(nat, [(a, 16, 16, 3), (b, 16, 16, 1)], 2, out, 32, 0, 1, 6, 6) == FQ_ERR_UNSUPPORTED          # up = 3
    assert _raw(nat, [(a, 16, 16, 2), (b, 16, 16, 1)], 2, out, 32, 0, 1, 7, 8) == FQ_ERR_UNSUPPORTED          # H % up != 0
    assert _raw(nat, [(a, 16, 16, 1), (b, 16, 16, 4)], 2, out, 32, 0, 1, 8, 6) == FQ_ERR_UNSUPPORTED          # W % up != 0
    assert _raw(nat, [(a, 16, 24, 1), (b, 16, 16, 1)], 2, out, 32, 0, 1, 4, 4) == FQ_ERR_UNSUPPORTED          # Cpad % 16 != 0
    assert _raw(nat, [(a, 16, 8, 1), (b, 16, 16, 1)], 2, out, 32, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG           # Cpad < C
    assert _raw(nat, ok2, 0, out, 32, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG                                       # nsrc 0
    assert _raw(nat, ok2 + [(b, 16, 16, 1)], 3, out, 48, 0, 1, 4, 4) == FQ_ERR_UNSUPPORTED                    # nsrc 3
    assert _raw(nat, [(a, 16, 16, 1)], 1, out, 16, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG                          # nothing to do
    assert _raw(nat, ok2, 2, out, 48, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG                                       # wrong Cpad_out
    assert _raw(nat, [(a, 20, 32, 1), (b, 20, 32, 1)], 2, out, 64, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG          # pad16(40) is 48, not 32 + 32
    assert _raw(nat, ok2, 2, None, 32, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG                                      # no output
    assert _raw(nat, [(None, 16, 16, 1), (b, 16, 16, 1)], 2, out, 32, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG       # no source
    assert _raw(nat, [(a, 0, 16, 1), (b, 16, 16, 1)], 2, out, 16, 0, 1, 4, 4) == FQ_ERR_INVALID_ARG           # C < 1
    L = nat.lib()
    ci2, ci3 = ctypes.c_int * 2, ctypes.c_int * 3
    assert L.fq_concat_i8_nhwc_supported(ci2(16, 16), ci2(1, 1), 2) == 1 and L.fq_concat_i8_nhwc_supported(ci2(3, 5), ci2(4, 2), 2) == 1
    assert L.fq_concat_i8_nhwc_supported(ci2(16, 16), ci2(1, 3), 2) == 0 and L.fq_concat_i8_nhwc_supported(ci2(16, 0), ci2(1, 1), 2) == 0
    assert L.fq_concat_i8_nhwc_supported(ci3(16, 16, 16), ci3(1, 1, 1), 3) == 0 and L.fq_concat_i8_nhwc_supported(ci2(16, 16), ci2(1, 1), 0) == 0
    torch.cuda.synchronize()
    assert bool((out == 5).all())                                   # nothing was launched
    assert _raw(nat, ok2, 2, out[..., :32].contiguous(), 32, 0, 1, 8, 8) == 0
    assert _raw(nat, [(a, 16, 16, 1)], 1, out[..., :16].contiguous(), 16, 1, 1, 8, 8) == 0          # a ReLU alone is work
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. modules: Fire, Concat + ReLU, FPN necks, Concat -> NewAdd
def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def _same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _check_forwards(net, x, plain):
    with torch.no_grad():
        assert _same(net(x), plain)
        assert _same(net(x[:1]), tuple(p[:1] for p in _tuple(plain)))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in _tuple(plain)))


NETS = {
    "fire": (lambda: cn.FireNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "cat_relu": (lambda: cn.CatReluNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "cat_relu_dim_by_name": (lambda: cn.CatReluNet(dim_by_name=True), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "fpn": (lambda: cn.FpnNet(), dict(resident_concats=1, resident_upsamples=1, fused_upsamples=1)),
    "fpn_x4": (lambda: cn.FpnNet(up=nn.Upsample(scale_factor=4, mode="nearest"), factor=4, coarse_c=5),
               dict(resident_concats=1, resident_upsamples=1, fused_upsamples=1)),
    "fpn_shared": (lambda: cn.FpnNet(shared=True), dict(resident_concats=1, resident_upsamples=1, fused_upsamples=0)),
    "cat_add": (lambda: cn.CatAddNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_modules_with_the_concat_plan(nat, tag):
    from common.quantity import resident
    make, want = NETS[tag]
    net, x = make().cuda().eval(), cn.example().cuda()
    with torch.no_grad():
        plain = net(x)
    assert all(float(p.abs().max()) > 0 for p in _tuple(plain))
    # without the argument: today's plan -- the branches write fp32 for the foreign Concat, no new summary keys
    off = resident.enable(net, x)
    plans = resident.describe(net)
    assert set(off) == cn.DEFAULT_KEYS and "cat" not in plans and "up" not in plans
    assert all(plans[n].emit_f32 for n in net.branches), plans
    _check_forwards(net, x, plain)

    on = resident.enable(net, x, concat=True)                              # verify=True
    plans = resident.describe(net)
    assert on["resident_concats"] >= 1 and {k: on[k] for k in want} == want, on
    assert all(plans[n].emit_f32 is False for n in net.branches), plans
    assert plans["cat"].emit_int and not plans["cat"].emit_f32
    if tag.startswith("fpn"):
        assert on["resident_upsamples"] >= 1 and plans["up"].up == (4 if tag == "fpn_x4" else 2)
        assert plans["up"].defer == (tag != "fpn_shared") and on["fused_upsamples"] == (0 if tag == "fpn_shared" else 1)
    if tag == "cat_add":
        assert plans["add"].resident_add and on["resident_adds"] == 1
    _check_forwards(net, x, plain)
    resident.disable(net)
    assert "forward" not in net.cat.__dict__ and not resident.describe(net)
    _check_forwards(net, x, plain)


DECLINED = {
    "bits_4_and_3": lambda: cn.CatReluNet(bits=(4, 3)),
    "add_sum_as_operand": lambda: cn.CatAddNet(add_operand=True),
    "dim_0": lambda: cn.CatReluNet(dim=0),
    "scale_factor_3": lambda: cn.FpnNet(up=nn.Upsample(scale_factor=3), factor=3),
    "bilinear": lambda: cn.FpnNet(up=nn.Upsample(scale_factor=2, mode="bilinear")),
}


@pytest.mark.parametrize("tag", sorted(DECLINED))
def test_declined_plans_keep_the_fp32_form(nat, tag):
    from common.quantity import resident
    net, x = DECLINED[tag]().cuda().eval(), cn.example().cuda()
    with torch.no_grad():
        plain = net(x)
    on = resident.enable(net, x, concat=True)
    plans = resident.describe(net)
    assert on["resident_concats"] == 0 and "cat" not in plans and "forward" not in net.cat.__dict__, (on, plans)
    if tag in ("scale_factor_3", "bilinear"):
        assert on["resident_upsamples"] == 0 and "up" not in plans and "forward" not in net.up.__dict__ and plans["coarse"].emit_f32
    elif tag == "add_sum_as_operand":
        assert plans["add"].emit_f32 and plans["c"].emit_f32
    else:
        assert all(plans[n].emit_f32 for n in net.branches)
    with torch.no_grad():
        assert _same(net(x), plain)
        if tag != "dim_0":
            assert _same(net(x[:1]), plain[:1])


# ---------------------------------------------------------------- 4. calibrated models end to end
def _fires(info):
    return sorted(n[:-len(".Concat")] for n in info if n.endswith(".Concat"))


@pytest.mark.parametrize("tag", ["tiny_concat", "squeezenet_32", "squeezenet_64"])
def test_calibrated_models_with_the_concat_plan(nat, tag, monkeypatch, tmp_path):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    if tag == "tiny_concat":
        fn, size = (lambda: cases.seed_model(cases.tiny_concat_net()).eval()), 8
        monkeypatch.setattr(torch, "save", lambda *a, **k: None)           # the fixture net is a local class: not picklable
    else:
        size = int(tag.split("_")[1])
        fn = lambda: cn.squeezenet(size)
    shape = (4, 3, size, size)
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(fn().cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        rec = Reconstruction(fn())
        info = rec.get_quantity_information()
        net = rec.ReconModel(info, os.path.join(wd, "recon_cat.pth")).cuda()
        # the Concat merge group gave both branches one bit
        if tag == "tiny_concat":
            pairs = [("branch_a", "branch_b")]
        else:
            pairs = [(f + ".expand1x1", f + ".expand3x3") for f in _fires(info)]
            assert len(pairs) == 8
        for a, b in pairs:
            assert info[a]["output_bit"] == info[b]["output_bit"], (a, b, info[a], info[b])
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0
        off = resident.enable(net, x)
        plans = resident.describe(net)
        assert all(plans[a].emit_f32 and plans[b].emit_f32 for a, b in pairs)
        with torch.no_grad():
            off_out = net(x)
        on = resident.enable(net, x, concat=True)                          # verify=True
        plans = resident.describe(net)
        print("%s: off %s; on %s" % (tag, off, on))
        assert on["resident_concats"] >= 1
        if tag != "tiny_concat":
            assert on["resident_concats"] == 8 and all(not plans[a].emit_f32 and not plans[b].emit_f32 for a, b in pairs)
            assert on["resident_pools"] >= 3 and on["fp32_outputs"] < off["fp32_outputs"]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(off_out, plain)
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        if tag != "tiny_concat":                                           # save / load round trip of the planned model
            path = str(tmp_path / "planned.pth")
            monkeypatch.undo()
            torch.save(net, path)
            again = torch.load(path, weights_only=False)
            assert resident.is_enabled(again) and len(resident.describe(again)) == len(plans)
            with torch.no_grad():
                assert torch.equal(again(x), plain)
        resident.disable(net)
        cat = [m for m in net.modules() if type(m).__name__ == "Concat"]
        assert cat and all("forward" not in m.__dict__ for m in cat) and not resident.describe(net)
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 5. HIP-graph capture of the plan
def test_hipgraph_capture_of_a_concat_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for make, key in ((cn.FireNet, "resident_concats"), (cn.FpnNet, "fused_upsamples"), (lambda: cn.FpnNet(shared=True), "resident_upsamples")):
        net = make().cuda().eval()
        x, x2 = cn.example(seed=1).cuda(), cn.example(seed=2).cuda() * 1.5
        with torch.no_grad():
            want, want2 = tuple(t.clone() for t in _tuple(net(x))), tuple(t.clone() for t in _tuple(net(x2)))
        assert not _same(want, want2)
        summary = resident.enable(net, x, concat=True)
        assert summary[key] >= 1 and summary["resident_concats"] >= 1
        graphed = resident.capture(net, x)
        assert _same(graphed(x), want)
        assert _same(graphed(x2), want2)
        assert _same(graphed(x), want)
        with torch.no_grad():
            assert _same(net(x2), want2)


# ---------------------------------------------------------------- 6. the model at the benchmark's size
def test_squeezenet_224_256_images_on_equals_off_equals_plain(nat):
    """Synthetic bits (no calibration): output bits from one float forward's abs-max, the two expand layers of a Fire module on
    the smaller of their two bits, input bit = the producer's output bit (concat_nets.squeezenet_info)."""
    from common.quantity import resident
    float_model = cn.squeezenet(224, classes=100)
    x = cases.fixed_input((256, 3, 224, 224)).cuda()
    bits = dn.measured_out_bits(copy.deepcopy(float_model).cuda(), x[:8])
    net = dn.rebuild(float_model, cn.squeezenet_info(float_model, bits)).cuda()
    with torch.no_grad():
        plain = net(x)
    assert float(plain.std(dim=0).max()) > 0                               # the images are told apart
    off = resident.enable(net, x, verify=False)
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    on = resident.enable(net, x, verify=False, concat=True)
    print("squeezenet 224: off %s; on %s" % (off, on))
    assert on["resident_concats"] == 8 and on["fp32_outputs"] < off["fp32_outputs"]
    with torch.no_grad():
        assert torch.equal(net(x), plain)
