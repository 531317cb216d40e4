"""Concatenation of up to eight resident int8 activations in one launch (fq_concat_n_i8_nhwc, csrc/fq_concat_i8.hip) against the
index rule in NumPy, and resident.enable(..., concat=True, flatten=True) on nets with nested Concats and on calibrated models.
Everything is integers: every comparison is exact.   pytest -m gpu"""
import copy
import ctypes
import io
import json
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

import avgpool_nets as an
import cases
import concat_n_nets as nn_
import concat_nets as cn
import depthwise_nets as dn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = 0, -1, -4
SENTINEL, GUARD = 0x5A, 64


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------- 1. the kernel against the index rule
@pytest.mark.parametrize("case", nn_.KERNEL_CASES, ids=nn_.case_id)
def test_concat_n_kernel_vs_index_rule(nat, case):
    rng = np.random.default_rng(sum(case[:3]) + sum((i + 1) * c for i, c in enumerate(case[3])) + sum(case[4]))
    arrays = nn_.sources(rng, case)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    total = sum(case[3])
    for relus in nn_.relu_patterns(case):
        want = nn_.index_rule(case, arrays, relus)
        srcs = [(d, C, u, r) for d, C, u, r in zip(dev, case[3], case[4], relus)]
        # the output is a view inside a larger buffer: sentinel bytes in front of and behind it must survive
        buf = torch.full((GUARD + want.size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
        view = buf[GUARD:GUARD + want.size].view(want.shape)
        assert view.data_ptr() % 16 == 0
        got = nat.concat_n_i8_nhwc(srcs, out=view)
        assert got is view
        head, body, tail = buf[:GUARD].cpu().numpy(), view.cpu().numpy(), buf[GUARD + want.size:].cpu().numpy()
        assert np.array_equal(body, want), (case, relus, np.argwhere(body != want)[:4])
        assert (head == SENTINEL).all() and (tail == SENTINEL).all()
        assert not body[..., total:].any()                                  # the padding channels are zero
        if want.size < (1 << 20):
            own = nat.concat_n_i8_nhwc(srcs)                                # ... and the allocating form
            assert tuple(own.shape) == want.shape and own.shape[-1] == nn_.pad16(total)
            assert np.array_equal(own.cpu().numpy(), want)
    for a, d in zip(arrays, dev):
        assert np.array_equal(d.cpu().numpy(), a)                           # the sources are only read


@pytest.mark.parametrize("case", nn_.OLD_CASES, ids=nn_.case_id)
def test_one_and_two_sources_equal_the_two_source_kernel(nat, case):
    rng = np.random.default_rng(17 + sum(case[:3]) + sum(case[3]))
    dev = [torch.from_numpy(a).cuda() for a in nn_.sources(rng, case)]
    for relu in (False, True):
        if not relu and len(dev) == 1 and case[4][0] == 1:
            continue
        old = nat.concat_i8_nhwc([(d, C, u) for d, C, u in zip(dev, case[3], case[4])], relu)
        new = nat.concat_n_i8_nhwc([(d, C, u, relu) for d, C, u in zip(dev, case[3], case[4])])
        assert old.shape == new.shape and torch.equal(old, new), (case, relu)


def test_the_case_list_covers_each_path_it_claims(tmp_path):
    exe = str(tmp_path / "concat_geom_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "concat_geom_check.cpp")])
    out = subprocess.run([exe] + [nn_.case_arg(c) for c in nn_.KERNEL_CASES], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    nn_.check_paths_reached(nn_.class_rows(out.stdout.splitlines()))


# ---------------------------------------------------------------- 2. what the entry point declines
def _raw(nat, srcs, nsrc, out, cpad_out, N, H, W):
    arr = (nat._CatSrcN * max(len(srcs), 1))()
    for i, (q, C, cpad, up, relu) in enumerate(srcs):
        ptr = q if isinstance(q, int) or q is None else q.data_ptr()
        arr[i].q, arr[i].C, arr[i].Cpad, arr[i].up, arr[i].relu = ptr, C, cpad, up, relu
    optr = out if isinstance(out, int) or out is None else out.data_ptr()
    return nat.lib().fq_concat_n_i8_nhwc(arr, nsrc, ctypes.c_void_p(optr) if optr is not None else None, cpad_out, N, H, W, None)


def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any of these geometries that could launch, and nothing may be
    launched."""
    a = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    b = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    c = torch.zeros(1, 8, 8, 32, dtype=torch.int8, device="cuda")
    out = torch.full((1, 8, 8, 160), 5, dtype=torch.int8, device="cuda")
    A, B, C = (a, 16, 16, 1, 0), (b, 16, 16, 1, 0), (c, 16, 16, 1, 0)
    ok3 = [A, B, C]
    INV, UNS = FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED
    assert _raw(nat, ok3, 0, out, 48, 1, 4, 4) == INV                                                  # nsrc < 1
    assert _raw(nat, ok3, -1, out, 48, 1, 4, 4) == INV
    assert nat.lib().fq_concat_n_i8_nhwc(None, 3, ctypes.c_void_p(out.data_ptr()), 48, 1, 4, 4, None) == INV
    assert _raw(nat, [A] * 9, 9, out, 144, 1, 4, 4) == UNS                                             # nsrc > 8
    assert _raw(nat, ok3, 3, None, 48, 1, 4, 4) == INV                                                 # no output
    assert _raw(nat, ok3, 3, out.data_ptr() + 8, 48, 1, 4, 4) == INV                                   # misaligned output
    assert _raw(nat, [A, (None, 16, 16, 1, 0), C], 3, out, 48, 1, 4, 4) == INV                         # no source
    assert _raw(nat, [A, B, (c.data_ptr() + 4, 16, 16, 1, 0)], 3, out, 48, 1, 4, 4) == INV             # misaligned source
    assert _raw(nat, [A, (b, 0, 16, 1, 0), C], 3, out, 32, 1, 4, 4) == INV                             # C < 1
    assert _raw(nat, [A, (b, 16, 16, 0, 0), C], 3, out, 48, 1, 4, 4) == INV                            # up < 1
    assert _raw(nat, [A, (b, 16, 8, 1, 0), C], 3, out, 48, 1, 4, 4) == INV                             # Cpad < C
    assert _raw(nat, [A, (b, 16, 16, 1, 2), C], 3, out, 48, 1, 4, 4) == INV                            # relu outside {0, 1}
    assert _raw(nat, [A, (b, 16, 16, 1, -1), C], 3, out, 48, 1, 4, 4) == INV
    assert _raw(nat, ok3, 3, out, 64, 1, 4, 4) == INV                                                  # wrong Cpad_out
    assert _raw(nat, [(a, 20, 32, 1, 0), (b, 20, 32, 1, 0), (c, 3, 16, 1, 0)], 3, out, 80, 1, 4, 4) == INV     # pad16(43) is 48
    assert _raw(nat, [A], 1, out, 16, 1, 4, 4) == INV                                                  # nothing to do
    assert _raw(nat, [A, (b, 16, 16, 3, 0), C], 3, out, 48, 1, 6, 6) == UNS                            # another factor
    assert _raw(nat, [A, (b, 16, 16, 8, 0), C], 3, out, 48, 1, 8, 8) == UNS
    assert _raw(nat, [A, (b, 16, 16, 2, 0), C], 3, out, 48, 1, 7, 8) == UNS                            # H % up != 0
    assert _raw(nat, [A, B, (c, 16, 16, 4, 0)], 3, out, 48, 1, 8, 6) == UNS                            # W % up != 0
    assert _raw(nat, [A, (b, 16, 24, 1, 0), C], 3, out, 48, 1, 4, 4) == UNS                            # Cpad % 16 != 0
    assert _raw(nat, [(a, 30000, 30000, 1, 0), (b, 30000, 30000, 1, 0), (c, 5537, 5552, 1, 0)], 3, out, 65552, 1, 1, 1) == UNS   # sum C > 65536
    assert _raw(nat, ok3, 3, out, 48, 1 << 12, 1 << 10, 1 << 10) == UNS                                # 2^31 - 1 bytes or more
    assert _raw(nat, [(a, 16, 1 << 20, 1, 0), B, C], 3, out, 48, 1, 64, 32) == UNS                     # ... a source (2^31 bytes exactly)
    assert _raw(nat, [(None, 16, 16, 1, 0)] * 3, 3, None, 48, 0, 4, 4) == FQ_OK                        # N == 0: no launch, no pointer read
    L = nat.lib()
    ci3, ci9 = ctypes.c_int * 3, ctypes.c_int * 9
    assert L.fq_concat_n_i8_nhwc_supported(ci3(16, 1, 30), ci3(1, 2, 4), 3) == 1 and L.fq_concat_n_i8_nhwc_supported(ci3(16, 16, 16), ci3(1, 3, 1), 3) == 0
    assert L.fq_concat_n_i8_nhwc_supported(ci9(*[16] * 9), ci9(*[1] * 9), 9) == 0 and L.fq_concat_n_i8_nhwc_supported(ci3(16, 16, 16), ci3(1, 1, 1), 0) == 0
    # the two-source function still declines three sources
    arr = (nat._CatSrc * 3)()
    for i, t in enumerate((a, b, c)):
        arr[i].q, arr[i].C, arr[i].Cpad, arr[i].up = t.data_ptr(), 16, 16, 1
    assert L.fq_concat_i8_nhwc(arr, 3, ctypes.c_void_p(out.data_ptr()), 48, 0, 1, 4, 4, None) == UNS
    torch.cuda.synchronize()
    assert bool((out == 5).all())                                   # nothing was launched
    o48 = torch.full((1, 8, 8, 48), 5, dtype=torch.int8, device="cuda")
    assert _raw(nat, ok3, 3, o48, 48, 1, 8, 8) == FQ_OK
    assert _raw(nat, [(a, 16, 16, 1, 1)], 1, torch.empty(1, 8, 8, 16, dtype=torch.int8, device="cuda"), 16, 1, 8, 8) == FQ_OK     # a ReLU alone is work
    torch.cuda.synchronize()
    assert not bool(o48.any())
    with pytest.raises(nat.FqError, match="different output planes"):
        nat.concat_n_i8_nhwc([(a, 16, 1, False), (b[:, :4].contiguous(), 16, 1, False), (c, 16, 1, False)])
    with pytest.raises(nat.FqError, match="no operand"):
        nat.concat_n_i8_nhwc([])


# ---------------------------------------------------------------- 3. nets with nested Concats
@pytest.mark.parametrize("tag", sorted(nn_.NETS))
def test_nested_concats_become_one_launch(nat, tag):
    """inception_block: one launch instead of three, flattened_concats == 2, logits on = off = plain bit for bit; spp; a chain of
    nine leaves keeps one inner Concat as its own launch; an inner ReLU under an outer Concat without (mixed flags); an inner
    Concat with a second reader and an upsampling between two Concats are not flattened (concat_n_nets.check_net)."""
    on = nn_.check_net(nat, tag, "cuda")
    assert on["flattened_concats"] == nn_.NETS[tag][1]
    if tag == "inception_block":
        assert on["flattened_concats"] == 2 and len(nn_.NETS[tag][3]) == 1


def test_a_deferred_concat_materialises_for_a_newadd_and_for_foreign_code(nat):
    from common.quantity import resident
    x = cn.example().cuda()
    net = nn_.NestedNet(inner_relu=True).cuda().eval()
    with torch.no_grad():
        plain = net(x)
        resident.enable(net, x, concat=True, flatten=True)
        s = net.r0(net.stem(x))
        a, b = net.a(s), net.b(s)
        d = net.r1(net.cat1(a, b))
        assert type(d) is resident.DeferredConcat and d._out is None and d.relu_done
        want = torch.relu(torch.cat([a.to_f32(), b.to_f32()], 1))
        assert torch.equal(resident.as_f32(d), want)                       # foreign code
        h = resident.resident_of(d)
        assert type(h) is resident.QHandle and h is d._out and tuple(h.shape) == (4, 16, 12, 12) and h.relu_done
        assert torch.equal(net.head(net.cat2(d, net.c(s))), plain)
        add_net = cn.CatAddNet().cuda().eval()
        plain_add = add_net(x)
        resident.enable(add_net, x, concat=True, flatten=True)
        s = add_net.r0(add_net.stem(x))
        d = resident.DeferredConcat([(add_net.a(s), 1, False), (add_net.b(s), 1, False)], 4)
        assert torch.equal(add_net.head(add_net.r1(add_net.add(d, add_net.c(s)))), plain_add) and d._out is not None


# ---------------------------------------------------------------- 4. golden G15 and calibrated models end to end
def test_g15_logits_equal_the_reference_with_flatten(nat, oracle, golden_dir):
    """The reference's own ReconModel logits of avgpool_nets.g15_net against the integer-simulation model on the HIP kernels with
    flatten=True: Concat2(Concat1(b1, b3), bp) over 8, 12 and 12 channels becomes one launch of the general family."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    with open(os.path.join(golden_dir, "g15_avgpool_net.json")) as fh:
        ref = json.load(fh)
    want = np.load(os.path.join(golden_dir, "g15_avgpool_net.npz"))["logits_recon"]
    shape = an.G15_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        q.activation_quantize(cases.calib_batches(3, shape, seed=an.G15_CALIB_SEED))
        q.weight_quantize()
        q.rewrite_weight()
        wd = os.path.join(tmp, "test", "workdir")
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon.pth")).cuda()
        x = cases.fixed_input(shape, seed=an.G15_INPUT_SEED).cuda()
        with nn_.Recorder(nat) as rec_calls, torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            off = resident.enable(net, x, concat=True, avgpool=True)
            on = resident.enable(net, x, concat=True, avgpool=True, flatten=True)
            rec_calls.calls[:] = []
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            assert rec_calls.calls == [(nn_.NSRC, [(8, 1, 0), (12, 1, 0), (12, 1, 0)])], rec_calls.calls
            np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on == dict(off, flattened_concats=1) and resident.describe(net).flattened_concats == ("Concat1",)


@pytest.mark.parametrize("size", [32, 64])
def test_calibrated_inception_with_flatten(nat, size, tmp_path):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    shape = (4, 3, size, size)
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(an.inception(size).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        rec = Reconstruction(an.inception(size))
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon_flat.pth")).cuda()
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0
        off = resident.enable(net, x, concat=True, avgpool=True)
        with torch.no_grad():
            off_out = net(x)
        with nn_.Recorder(nat) as rec_calls:
            on = resident.enable(net, x, concat=True, avgpool=True, flatten=True)  # verify=True
            plans = resident.describe(net)
            print("inception %d: off %s; on %s" % (size, off, on))
            assert on == dict(off, flattened_concats=on["flattened_concats"]) and on["flattened_concats"] >= 2
            assert len(plans.flattened_concats) == on["flattened_concats"]
            rec_calls.calls[:] = []
            with torch.no_grad():
                assert torch.equal(net(x), plain) and torch.equal(off_out, plain)
            assert len(rec_calls.calls) == on["resident_concats"] - on["flattened_concats"]
            assert any(name == nn_.NSRC and len(ops) == 4 for name, ops in rec_calls.calls), rec_calls.calls
            with torch.no_grad():
                assert torch.equal(net(x[:1]), plain[:1])
                assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        path = str(tmp_path / "planned.pth")                                    # save / load round trip of the planned model
        torch.save(net, path)
        again = torch.load(path, weights_only=False)
        assert resident.is_enabled(again) and nn_.rows(again) == nn_.rows(net)
        assert resident.describe(again).flattened_concats == plans.flattened_concats
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        buf = io.BytesIO()
        pickle.dump(net, buf)
        third = pickle.loads(buf.getvalue())
        with torch.no_grad():
            assert torch.equal(third(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 5. HIP-graph capture of the plan
def test_hipgraph_capture_of_a_flattened_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for tag in ("inception_block", "inner_relu"):
        net = nn_.NETS[tag][0]().cuda().eval()
        x, x2 = cn.example(seed=1).cuda(), cn.example(seed=2).cuda() * 1.5
        with torch.no_grad():
            want, want2 = tuple(t.clone() for t in nn_._tuple(net(x))), tuple(t.clone() for t in nn_._tuple(net(x2)))
        assert not nn_.same(want, want2)
        summary = resident.enable(net, x, concat=True, avgpool=True, flatten=True)
        assert summary["flattened_concats"] == nn_.NETS[tag][1]
        graphed = resident.capture(net, x)
        assert nn_.same(graphed(x), want)
        assert nn_.same(graphed(x2), want2)
        assert nn_.same(graphed(x), want)
        with torch.no_grad():
            assert nn_.same(net(x2), want2)


# ---------------------------------------------------------------- 6. the model at the cost script's size
def test_inception_224_256_images_on_equals_off(nat):
    """Synthetic bits (no calibration; avgpool_nets.inception_info): all twelve Concats are planned, eight are flattened, four
    launches of the aligned family remain.  One forward per arm."""
    from common.quantity import resident
    float_model = an.inception(224, classes=100)
    x = cases.fixed_input((256, 3, 224, 224)).cuda()
    bits = dn.measured_out_bits(copy.deepcopy(float_model).cuda(), x[:8])
    net = dn.rebuild(float_model, an.inception_info(float_model, bits)).cuda()
    off = resident.enable(net, x, verify=False, concat=True, avgpool=True)
    with torch.no_grad():
        off_out = net(x)
    assert float(off_out.std(dim=0).max()) > 0                                 # the images are told apart
    on = resident.enable(net, x, verify=False, concat=True, avgpool=True, flatten=True)
    print("inception 224: off %s; on %s" % (off, on))
    assert on == dict(off, flattened_concats=8) and on["resident_concats"] == 12
    with nn_.Recorder(nat) as rec_calls, torch.no_grad():
        assert torch.equal(net(x), off_out)
    assert len(rec_calls.calls) == 4 and all(name == nn_.NSRC and len(ops) == 4 for name, ops in rec_calls.calls)
