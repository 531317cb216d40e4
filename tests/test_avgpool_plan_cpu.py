"""resident.enable(..., avgpool=True) on a box without a GPU: the tracer, the plan, the handles and the module glue run for real;
the kernel entry points are oracle-backed doubles (tests/native_doubles.py, concat_doubles.py, avgpool_doubles.py) that follow the
reference's fp32 chain literally.  Every comparison is exact.  The rule of include/fq.h (fq_avgpool_i8_nhwc) is held against
torch's own chain, the kernel's address arithmetic is walked on the host over the GPU tests' shape list
(scripts/avgpool_geom_check.cpp), and golden G15 pins a calibrated net with both pools to the reference."""
import io
import json
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import avgpool_doubles
import avgpool_nets as an
import cases
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = {"resident_concats", "resident_upsamples", "fused_upsamples", "resident_avgpools"}


def _plans(model):
    from common.quantity import resident
    return resident.describe(model)


def _rows(model):
    from common.quantity import resident
    return {n: tuple(getattr(p, f) for f in p.__slots__) for n, p in resident.describe(model).items()}


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


# ---------------------------------------------------------------- 1. the rule
def _torch_chain(x, C, kernel, stride, padding, cip, g, b, relu):
    """DeQuantity(g) -> nn.AvgPool2d -> nn.ReLU -> Quantity(b) with torch's CPU operators, on int8 NHWC."""
    f = torch.from_numpy(x[..., :C].astype(np.float32)).permute(0, 3, 1, 2).contiguous() * float(2.0 ** -g)
    y = nn.AvgPool2d(kernel, stride, padding, ceil_mode=False, count_include_pad=cip)(f)
    if relu:
        y = torch.relu(y)
    q = torch.clamp(torch.round(y * float(2.0 ** b)), -128, 127)
    out = np.zeros(tuple(q.shape[:1]) + tuple(q.shape[2:]) + (x.shape[-1],), np.int8)
    out[..., :C] = q.permute(0, 2, 3, 1).numpy().astype(np.int8)
    return out


@pytest.mark.parametrize("case", an.KERNEL_CASES, ids=an.case_arg)
def test_the_numpy_rule_is_torchs_chain(case):
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    C, kernel, stride, padding = case[3], case[4:6], case[6:8], case[8:10]
    checked = 0
    for kind in ("random", "max", "min"):
        x = an.source(rng, case, kind)
        for cip in (False, True):
            for relu in (False, True):
                for n, shift in enumerate(an.SHIFTS):
                    g = (0, 4, -2, 7, 3)[n]
                    want = _torch_chain(x, C, kernel, stride, padding, cip, g, g + shift, relu)
                    got = an.numpy_rule(x, C, kernel, stride, padding, cip, shift, relu)
                    np.testing.assert_array_equal(got, want, err_msg=str((kind, cip, relu, shift)))
                    checked += got[..., :C].size
    assert checked > 0


def test_the_rule_rounds_ties_to_even_and_the_double_follows_it():
    x = an.tie_source()
    with avgpool_doubles.installed():
        for shift, want in ((0, [[0, 2, 2], [0, -2, -2], [1, 3, -1]]), (-1, [[0, 1, 1], [0, -1, -1], [0, 2, 0]])):
            got = an.numpy_rule(x, 16, (2, 2), (2, 2), (0, 0), True, shift, False)
            assert got[0, :, :, 0].tolist() == want and (got == got[..., :1]).all()
            dbl = avgpool_doubles.avgpool_i8_nhwc(torch.from_numpy(x), 16, (2, 2), (2, 2), (0, 0), True, shift, False)
            np.testing.assert_array_equal(dbl.numpy(), got)
            np.testing.assert_array_equal(_torch_chain(x, 16, (2, 2), (2, 2), (0, 0), True, 3, 3 + shift, False), got)


def test_the_double_is_the_rule_on_the_case_list():
    with avgpool_doubles.installed():
        for case in an.KERNEL_CASES:
            rng = np.random.default_rng(7 + sum(case))
            x = an.source(rng, case)
            for cip, relu, shift in ((True, False, 0), (False, True, 1), (False, False, -8), (True, True, 8)):
                got = avgpool_doubles.avgpool_i8_nhwc(torch.from_numpy(x), case[3], case[4:6], case[6:8], case[8:10], cip, shift, relu)
                np.testing.assert_array_equal(got.numpy(), an.numpy_rule(x, case[3], case[4:6], case[6:8], case[8:10], cip, shift, relu))


# ---------------------------------------------------------------- 2. what is planned
NETS = {
    "inception_block": (lambda: an.InceptionBlockNet(), dict(resident_avgpools=1, resident_concats=3)),
    "transition": (lambda: an.PoolNet(), dict(resident_avgpools=1)),
    "relu_behind": (lambda: an.PoolNet(relu_behind=True), dict(resident_avgpools=1)),
    "two_readers": (lambda: an.PoolNet(pool=nn.AvgPool2d(3, 1, 1, count_include_pad=False), read_bits=(4, 4)), dict(resident_avgpools=1)),
    "reader_at_another_bit": (lambda: an.PoolNet(read_bits=(3,)), dict(resident_avgpools=1)),
    "rectangular": (lambda: an.PoolNet(pool=nn.AvgPool2d((2, 3), (1, 2), (1, 1))), dict(resident_avgpools=1)),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_windowed_pools_become_integer_layers(tag):
    from common.quantity import resident
    make, want = NETS[tag]
    with avgpool_doubles.installed() as nat:
        net, x = make().eval(), an.example()
        with torch.no_grad():
            plain = net(x)
        assert all(float(p.abs().max()) > 0 for p in _tuple(plain))
        # without the argument: the parent's plan, field for field -- the pool is foreign code and its source writes fp32
        a = resident.enable(net, x, concat=True)
        rows = _rows(net)
        b = resident.enable(net, x, concat=True, avgpool=False)
        assert a == b and rows == _rows(net) and set(a) == an.DEFAULT_KEYS | (NEW_KEYS - {"resident_avgpools"})
        off_plans = _plans(net)
        assert "pool" not in off_plans and "forward" not in net.pool.__dict__
        assert all(off_plans[n].emit_f32 for n in net.sources), off_plans
        _check_forwards(net, x, plain)

        calls = []
        real = nat.avgpool_i8_nhwc
        nat.avgpool_i8_nhwc = lambda *args, **kw: (calls.append(args[1:]), real(*args, **kw))[1]
        try:
            on = resident.enable(net, x, concat=True, avgpool=True)            # verify=True: bit-identical to the traced forward
            plans = _plans(net)
            assert set(on) == an.DEFAULT_KEYS | NEW_KEYS and {k: on[k] for k in want} == want, on
            for n in net.sources:
                assert plans[n].emit_int and not plans[n].emit_f32, (n, plans[n])
            p = plans["pool"]
            assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolWindowResident)
            assert p.emit_int and not p.emit_f32 and p.grid == 4 and p.narrow_bit == (3 if tag == "reader_at_another_bit" else 4)
            assert on["resident_convs"] == a["resident_convs"] and on["fp32_outputs"] == a["fp32_outputs"] - len(net.sources)
            calls[:] = []
            _check_forwards(net, x, plain)
            assert len(calls) == 3
            if tag == "inception_block":
                assert calls[0] == (16, (3, 3), (1, 1), (1, 1), True, 0, False) and not p.relu and plans["bp"].relu
                assert all(plans[c].emit_int and not plans[c].emit_f32 for c in ("cat1", "cat2", "cat3"))
            if tag == "transition":
                assert calls[0] == (16, (2, 2), (2, 2), (0, 0), True, 0, False) and plans["stem"].relu
            if tag == "relu_behind":
                assert p.relu and not plans["stem"].relu and calls[0] == (16, (2, 2), (2, 2), (0, 0), True, 0, True)
                assert isinstance(net.r1.__dict__["forward"], resident._ReluPassThrough)
            if tag == "two_readers":
                assert calls[0] == (16, (3, 3), (1, 1), (1, 1), False, 0, False)
            if tag == "reader_at_another_bit":
                assert calls[0][5] == -1
            if tag == "rectangular":
                assert calls[0] == (16, (2, 3), (1, 2), (1, 1), True, 0, False)
            # the handle carries the narrow payload only
            with torch.no_grad():
                s = net.stem(x) if tag == "relu_behind" else net.r0(net.stem(x))
                h = net.pool(s)
            assert type(h) is resident.QHandle and h.exact is None and h.grid is None and h.narrow.dtype == torch.int8
            assert h.bit == p.narrow_bit and tuple(h.shape) == (4, 16) + tuple(h.narrow.shape[1:3]) and h.relu_done
            with pytest.raises(nat.FqError):
                h.to_f32()
            resident.disable(net)
            assert not _plans(net) and all("forward" not in m.__dict__ for m in net.modules())
            calls[:] = []
            with torch.no_grad():
                assert _same(net(x), plain)
            assert not calls
        finally:
            nat.avgpool_i8_nhwc = real


def test_the_default_call_is_the_parents():
    """enable(net, x) and enable(net, x, avgpool=False): no new summary key, no plan for the pool, the same rows."""
    from common.quantity import resident
    with avgpool_doubles.installed():
        for make in (an.InceptionBlockNet, an.PoolNet):
            net, x = make().eval(), an.example()
            a = resident.enable(net, x)
            rows = _rows(net)
            b = resident.enable(net, x, avgpool=False)
            assert a == b and rows == _rows(net) and set(a) == an.DEFAULT_KEYS
            assert "pool" not in _plans(net) and _plans(net)["stem"].emit_f32
            c = resident.enable(net, x, avgpool=True)                          # the switch alone, without the Concat plan
            assert set(c) == an.DEFAULT_KEYS | {"resident_avgpools"} and c["resident_avgpools"] == 1


DECLINED = {
    "add_sum_as_source": lambda: an.PoolNet(mode="add_source"),
    "two_bits": lambda: an.PoolNet(read_bits=(4, 3)),
    "concat_consumer": lambda: an.PoolNet(pool=nn.AvgPool2d(3, 1, 1), mode="concat"),
    "maxpool_consumer": lambda: an.PoolNet(mode="maxpool"),
    "foreign_consumer": lambda: an.PoolNet(mode="foreign"),
    "ceil_mode": lambda: an.PoolNet(pool=nn.AvgPool2d(2, ceil_mode=True)),
    "divisor_override": lambda: an.PoolNet(pool=nn.AvgPool2d(2, divisor_override=3)),
    "window_9x9": lambda: an.PoolNet(pool=nn.AvgPool2d(9, 1, 4)),
    "shift_9": lambda: an.PoolNet(src_bit=-2, read_bits=(7,)),
    "shift_minus_9": lambda: an.PoolNet(src_bit=7, read_bits=(-2,)),
    "called_twice": lambda: an.PoolNet(mode="twice"),
}


@pytest.mark.parametrize("tag", sorted(DECLINED))
def test_what_the_plan_declines_stays_in_fp32_form(tag):
    from common.quantity import resident
    with avgpool_doubles.installed() as nat:
        net, x = DECLINED[tag]().eval(), an.example()
        with torch.no_grad():
            plain = net(x)
        calls = []
        real = nat.avgpool_i8_nhwc
        nat.avgpool_i8_nhwc = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            off = resident.enable(net, x, concat=True)
            rows = _rows(net)
            on = resident.enable(net, x, concat=True, avgpool=True)
            plans = _plans(net)
            assert on["resident_avgpools"] == 0 and "pool" not in plans and "forward" not in net.pool.__dict__, (on, plans)
            assert rows == _rows(net) and {k: v for k, v in on.items() if k != "resident_avgpools"} == off
            src = "add" if tag == "add_sum_as_source" else "stem"
            assert plans[src].emit_f32, plans[src]
            _check_forwards(net, x, plain)
            assert not calls
        finally:
            nat.avgpool_i8_nhwc = real


def test_the_forward_stays_adaptive():
    """A planned pool that meets an input it was not planned for falls back to torch on fp32."""
    from common.quantity import resident
    with avgpool_doubles.installed() as nat:
        net, x = an.PoolNet().eval(), an.example()
        resident.enable(net, x, avgpool=True)
        calls = []
        real = nat.avgpool_i8_nhwc
        nat.avgpool_i8_nhwc = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            with torch.no_grad():
                s = net.r0(net.stem(x))
                assert type(s) is resident.QHandle
                f = s.to_f32()
                want = nn.functional.avg_pool2d(f, 2)
                assert torch.equal(net.pool(f), want) and not calls                       # an fp32 tensor without a handle
                other = resident.QHandle(s.shape, s.exact, s.grid + 1, s.narrow, s.bit + 1, s.relu_done)
                assert torch.equal(net.pool(other), nn.functional.avg_pool2d(other.to_f32(), 2)) and not calls      # another grid
                net.pool.kernel_size, net.pool.stride = 9, 1                              # a window the kernel declines
                net.pool.padding = 4
                assert torch.equal(net.pool(s), nn.functional.avg_pool2d(f, 9, 1, 4)) and not calls
                net.pool.kernel_size, net.pool.stride, net.pool.padding = 2, 2, 0
                assert type(net.pool(s)) is resident.QHandle and len(calls) == 1
                plan = net.pool.__dict__.pop("_resident")
                assert torch.equal(net.pool(s), want) and len(calls) == 1                 # no plan
                net.pool.__dict__["_resident"] = plan
        finally:
            nat.avgpool_i8_nhwc = real


def test_the_whole_plane_pool_keeps_its_own_forward():
    from common.quantity import resident
    with avgpool_doubles.installed():
        net, x = an.GlobalPoolNet().eval(), an.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x)
        on = resident.enable(net, x, avgpool=True)
        assert isinstance(net.gpool.__dict__["forward"], resident._AvgPoolResident) and "gpool" not in _plans(net)
        assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolWindowResident)
        assert on["resident_avgpools"] == 1 and on["resident_pools"] == off["resident_pools"] == 1
        _check_forwards(net, x, plain)


def test_a_planned_model_pickles_with_its_plan():
    from common.quantity import resident
    with avgpool_doubles.installed():
        for make in (an.InceptionBlockNet, an.PoolNet):
            net, x = make().eval(), an.example()
            with torch.no_grad():
                plain = net(x)
            resident.enable(net, x, concat=True, avgpool=True)
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert _rows(again) == _rows(net) and isinstance(again.pool.__dict__["forward"], resident._AvgPoolWindowResident)
            with torch.no_grad():
                assert _same(again(x), plain)
            resident.disable(again)
            assert not _plans(again) and "forward" not in again.pool.__dict__


def test_avgpool_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.avgpool_supported
    assert ok((3, 3), (1, 1), (1, 1), 0) and ok((2, 2), (2, 2), (0, 0), -8) and ok((8, 8), (8, 8), (4, 4), 8) and ok((1, 64), (1, 1), (0, 32), 0)
    assert ok((2, 3), (1, 2), (1, 1), 1) and ok((7, 7), (1, 1), (3, 3), 0)
    assert not ok((9, 9), (1, 1), (4, 4), 0) and not ok((5, 13), (1, 1), (0, 0), 0) and not ok((65, 1), (1, 1), (0, 0), 0)
    assert not ok((3, 3), (1, 1), (1, 1), 9) and not ok((3, 3), (1, 1), (1, 1), -9)
    assert not ok((3, 3), (1, 1), (2, 1), 0) and not ok((3, 3), (1, 1), (1, 2), 0) and not ok((3, 3), (1, 1), (-1, 0), 0)
    assert not ok((0, 3), (1, 1), (0, 0), 0) and not ok((3, 3), (0, 1), (0, 0), 0) and not ok((3, 3), (1, -1), (0, 0), 0)
    assert not ok((65536, 65536), (1, 1), (0, 0), 0)


def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_avgpool_i8_geom.h holds the kernel's lane -> (chunk, taps, divisor, addresses) functions and compiles as host code:
    scripts/avgpool_geom_check.cpp walks every lane of every launch and exits non-zero on a load outside the source, an unaligned
    load, a tap that is not in window ∩ image or is loaded twice, a wrong divisor or an output chunk written twice or not at all --
    over its built-in list and over the GPU tests' shape list."""
    exe = str(tmp_path / "avgpool_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "avgpool_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
    shapes = an.KERNEL_CASES + [an.STRIDE_LOOP_CASE, (1, 6, 6, 16, 2, 2, 2, 2, 0, 0)]
    out = subprocess.run([exe] + [an.case_arg(c) for c in shapes], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(shapes) + 1, out.stdout + out.stderr
    stride_loop = [ln for ln in lines if ln.startswith("case " + an.case_arg(an.STRIDE_LOOP_CASE))][0].split()
    assert int(stride_loop[stride_loop.index("chunks") + 1]) > 2048 * 256 and int(stride_loop[stride_loop.index("blocks") + 1]) == 2048


# ---------------------------------------------------------------- 3. golden G15: a calibrated net with both pools
@pytest.fixture(scope="module")
def g15(golden_dir):
    with open(os.path.join(golden_dir, "g15_avgpool_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g15_avgpool_net.npz"))


def test_g15_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g15, oracle):
    """The reference's graph discovery, merge groups, feat.table and weight.table of avgpool_nets.g15_net byte for byte through
    the oracle-backed CPU engine, and its ReconModel logits bit for bit: plain, with the parent's plan and with avgpool=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g15
    shape = an.G15_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(cases.calib_batches(3, shape, seed=an.G15_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        # a convolution behind a pool reads at the bit of the pool's source
        assert info["bp"]["input_bit"] == info["stem"]["output_bit"] and info["trans"]["input_bit"] == info["bp"]["output_bit"]
        assert info["b1"]["output_bit"] == info["b3"]["output_bit"] == info["bp"]["output_bit"]
        with avgpool_doubles.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = cases.fixed_input(shape, seed=an.G15_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x, concat=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                on = resident.enable(net, x, concat=True, avgpool=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            plans = _plans(net)
            assert off["fp32_outputs"] - on["fp32_outputs"] == 2 and on["resident_avgpools"] == 2 and on["resident_concats"] == 2, (off, on)
            assert not plans["stem"].emit_f32 and not plans["Concat2"].emit_f32 and "pool_g" not in plans
            assert isinstance(net.pool_g.__dict__["forward"], resident._AvgPoolResident)
