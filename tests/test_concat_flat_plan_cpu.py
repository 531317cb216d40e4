"""resident.enable(..., concat=True, flatten=True) on a box without a GPU: the tracer, the plan, the handles and the module glue
run for real; the kernel entry points are doubles (tests/native_doubles.py, concat_doubles.py, avgpool_doubles.py and
concat_n_doubles.py, the rule of include/fq.h in torch).  Every comparison is exact.  The N-source kernel's address arithmetic
is walked on the host over the GPU tests' shape list (scripts/concat_geom_check.cpp), and the byte accounting of
scripts/concat_flat_cost.py is held against the closed form."""
import copy
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import avgpool_nets as an
import concat_n_doubles
import concat_n_nets as nn_
import concat_nets as cn
import depthwise_nets as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the double is the rule
def test_the_double_is_the_index_rule_on_the_case_list():
    small = [c for c in nn_.KERNEL_CASES if c not in nn_.STRIDED_CASES]
    for case in small:
        rng = np.random.default_rng(sum(case[:3]) + sum(case[3]))
        arrays = nn_.sources(rng, case)
        for relus in nn_.relu_patterns(case):
            got = concat_n_doubles.concat_n_i8_nhwc([(torch.from_numpy(a), C, u, r) for a, C, u, r in zip(arrays, case[3], case[4], relus)])
            np.testing.assert_array_equal(got.numpy(), nn_.index_rule(case, arrays, relus), err_msg=str((case, relus)))


def test_the_case_list_is_the_one_the_kernel_was_specified_on():
    assert len(nn_.ALIGNED_CASES) == 2 and len(nn_.GENERAL_CASES) == 5 and len(nn_.UPSAMPLED_CASES) == 4 and len(nn_.STRIDED_CASES) == 2
    assert len(nn_.OLD_CASES) == len(cn.TWO_SOURCE_CASES) + len(cn.ONE_SOURCE_CASES)
    for case in nn_.GENERAL_CASES:
        n = len(case[3])
        assert nn_.relu_patterns(case) == [[0] * n, [1] * n, [(i + 1) % 2 for i in range(n)]]
    for N, H, W, Cs, _ups in nn_.STRIDED_CASES:
        assert N * H * W * nn_.pad16(sum(Cs)) // 16 > 2048 * 256
    a, g = nn_.STRIDED_CASES
    assert nn_.pad16(sum(a[3])) // 16 == 16 and nn_.pad16(sum(g[3])) // 16 == 5 and (2048 * 256) % 5 != 0
    for N, H, W, Cs, _ups in set((c[0], c[1], c[2], tuple(c[3]), tuple(c[4])) for c in nn_.KERNEL_CASES) - set(
            (c[0], c[1], c[2], tuple(c[3]), tuple(c[4])) for c in nn_.STRIDED_CASES):
        assert N * H * W * nn_.pad16(sum(Cs)) < 300 * 1024


# ---------------------------------------------------------------- 2. what is planned, launched and with which operands
@pytest.mark.parametrize("tag", sorted(nn_.NETS))
def test_nested_concats_become_one_launch(tag):
    with concat_n_doubles.installed() as nat:
        on = nn_.check_net(nat, tag, "cpu")
        assert on["flattened_concats"] == nn_.NETS[tag][1]


def test_flatten_needs_the_concat_plan():
    from common.quantity import resident
    with concat_n_doubles.installed():
        net, x = an.InceptionBlockNet().eval(), an.example()
        with pytest.raises(ValueError):
            resident.enable(net, x, flatten=True)
        with pytest.raises(ValueError):
            resident.enable(net, x, avgpool=True, flatten=True)
        assert not resident.is_enabled(net) and not resident.describe(net)


def _all_parent_nets():
    import test_avgpool_plan_cpu as ta
    import test_concat_plan_cpu as tc
    nets = {}
    for mod, tables in ((tc, (tc.NETS, tc.DECLINED)), (ta, (ta.NETS, ta.DECLINED))):
        for table in tables:
            for tag, entry in table.items():
                nets["%s.%s" % (mod.__name__, tag)] = entry[0] if isinstance(entry, tuple) else entry
    nets["global_pool"] = an.GlobalPoolNet
    return nets


def test_with_the_switch_off_plans_and_summaries_are_todays():
    """The default call, concat=True alone and concat=True, avgpool=True on every net of test_concat_plan_cpu.py and
    test_avgpool_plan_cpu.py: flatten=False and the argument left out give the same summary dict and the same plan rows, no
    `flattened_concats` key, no deferred Concat, and only the two-source entry point is ever called."""
    from common.quantity import resident
    with concat_n_doubles.installed() as nat:
        for tag, make in sorted(_all_parent_nets().items()):
            net, x = make().eval(), cn.example()
            with torch.no_grad():
                plain = net(x)
            for kwargs, keys in ((dict(), cn.DEFAULT_KEYS),
                                 (dict(concat=True), cn.DEFAULT_KEYS | {"resident_concats", "resident_upsamples", "fused_upsamples"}),
                                 (dict(concat=True, avgpool=True), cn.DEFAULT_KEYS | {"resident_concats", "resident_upsamples",
                                                                                      "fused_upsamples", "resident_avgpools"})):
                a = resident.enable(net, x, **kwargs)
                rows = nn_.rows(net)
                b = resident.enable(net, x, flatten=False, **kwargs)
                assert a == b and set(a) == keys and rows == nn_.rows(net), (tag, kwargs, a, b)
                d = resident.describe(net)
                assert d.flattened_concats == () and not any(p.defer for n, p in d.items() if "cat" in n.lower()), (tag, kwargs)
                with nn_.Recorder(nat) as rec:
                    with torch.no_grad():
                        assert nn_.same(net(x), plain), (tag, kwargs)
                    assert all(name == nn_.TWO for name, _ops in rec.calls), (tag, rec.calls)
                    assert len(rec.calls) == (a.get("resident_concats", 0) + a.get("resident_upsamples", 0) - a.get("fused_upsamples", 0))
            resident.disable(net)


def test_a_foreign_reader_or_an_fp32_consumer_keeps_the_inner_concat():
    """What is not deferred, and why: a value that foreign code touches (emit_f32), and an inner Concat whose consumer is no
    resident Concat."""
    from common.quantity import resident

    class Foreign(nn_.NestedNet):
        def forward(self, x):
            s = self.r0(self.stem(x))
            inner = self.cat1(self.a(s), self.b(s))
            return self.head(self.cat2(inner, self.c(s))), inner * 2.0

    with concat_n_doubles.installed():
        net, x = Foreign().eval(), cn.example()
        with torch.no_grad():
            plain = net(x)
        on = resident.enable(net, x, concat=True, flatten=True)
        plans = resident.describe(net)
        assert on["flattened_concats"] == 0 and on["resident_concats"] == 2 and plans["cat1"].emit_f32 and not plans["cat1"].defer
        with torch.no_grad():
            assert nn_.same(net(x), plain)
        # operands on two grids: the outer Concat is not planned at all, the inner one has nobody to be deferred into
        net2 = nn_.NestedNet().eval()
        net2.c = cn.conv(16, 8, 1, 4, 3, seed=1)
        with torch.no_grad():
            plain2 = net2(x)
        on2 = resident.enable(net2, x, concat=True, flatten=True)
        assert on2["flattened_concats"] == 0 and on2["resident_concats"] == 1 and "cat2" not in resident.describe(net2)
        with torch.no_grad():
            assert nn_.same(net2(x), plain2)


def test_a_deferred_concat_materialises_for_anything_but_the_concat():
    from common.quantity import resident
    with concat_n_doubles.installed() as nat:
        net, x = nn_.NestedNet(inner_relu=True).eval(), cn.example()
        with torch.no_grad():
            plain = net(x)
            resident.enable(net, x, concat=True, flatten=True)
            s = net.r0(net.stem(x))
            a, b = net.a(s), net.b(s)
            with nn_.Recorder(nat) as rec:
                d = net.r1(net.cat1(a, b))
                assert type(d) is resident.DeferredConcat and d._out is None and not rec.calls and d.relu_done
                assert [(h.shape[1], up, r) for h, up, r in d.leaves] == [(8, 1, True), (8, 1, True)] and d.grid == 4
                want = torch.relu(torch.cat([a.to_f32(), b.to_f32()], 1))
                assert torch.equal(resident.as_f32(d), want)                   # fp32 for foreign code: one launch ...
                h = resident.resident_of(d)                                    # ... whose result is kept for the next reader
                assert type(h) is resident.QHandle and h is d._out and tuple(h.shape) == (4, 16, 12, 12) and h.relu_done and h.grid == 4
                assert rec.calls == [(nn_.TWO, [(8, 1, 1), (8, 1, 1)])]
                # a materialised operand is then read as an ordinary handle by the outer Concat, with the same result
                y = net.head(net.cat2(d, net.c(s)))
                assert torch.equal(y, plain) and rec.calls[1:] == [(nn_.TWO, [(16, 1, 0), (8, 1, 0)])]
            # a NewAdd that meets a DeferredConcat reads its integers
            add_net = cn.CatAddNet().eval()
            plain_add = add_net(x)
            resident.enable(add_net, x, concat=True, flatten=True)
            s = add_net.r0(add_net.stem(x))
            ha, hb = add_net.a(s), add_net.b(s)
            d = resident.DeferredConcat([(ha, 1, False), (hb, 1, False)], 4)
            assert torch.equal(add_net.head(add_net.r1(add_net.add(d, add_net.c(s)))), plain_add) and d._out is not None
            # a leaf on another grid: the deferred part is materialised and the fp32 path runs
            net3 = nn_.NestedNet().eval()
            plain3 = net3(x)
            resident.enable(net3, x, concat=True, flatten=True)
            s = net3.r0(net3.stem(x))
            d = net3.cat1(net3.a(s), net3.b(s))
            c = net3.c(s)
            other = resident.QHandle(c.shape, c.exact, c.grid + 1, c.narrow, c.bit + 1, c.relu_done)
            want = net3.head(torch.cat([d.to_f32(), other.to_f32()], 1))
            assert torch.equal(net3.head(net3.cat2(d, other)), want) and torch.equal(net3(x), plain3)


def test_a_planned_model_pickles_with_its_plan():
    from common.quantity import resident
    with concat_n_doubles.installed():
        for make in (an.InceptionBlockNet, nn_.SppNet):
            net, x = make().eval(), cn.example()
            with torch.no_grad():
                plain = net(x)
            resident.enable(net, x, concat=True, avgpool=True, flatten=True)
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert nn_.rows(again) == nn_.rows(net) and resident.describe(again).flattened_concats == resident.describe(net).flattened_concats
            assert resident.describe(again).flattened_concats
            with torch.no_grad():
                assert nn_.same(again(x), plain)
            resident.disable(again)
            assert not resident.describe(again)
    assert "defer" in resident.Plan.__slots__ and not any("flat" in s for s in resident.Plan.__slots__)      # Plan.defer is reused


def test_concat_n_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.concat_n_supported
    assert ok([16, 16], [1, 1]) and ok([3], [4]) and ok([1] * 8, [1, 2, 4, 1, 2, 4, 1, 2]) and ok([17, 1, 30], [1, 1, 1])
    assert ok([65536], [1]) and ok([65535, 1], [1, 1])
    assert not ok([16] * 9, [1] * 9) and not ok([], []) and not ok([16, 16], [1])
    assert not ok([16, 16, 16], [1, 3, 1]) and not ok([16, 16, 16], [1, 8, 1]) and not ok([16, 0, 16], [1, 1, 1])
    assert not ok([65536, 1], [1, 1]) and not ok([30000, 30000, 5537], [1, 1, 1])
    # the two-source answer is unchanged
    assert not _native.concat_supported([16, 16, 16], [1, 1, 1]) and _native.concat_supported([16, 16], [1, 1])
    assert _native.CONCAT_N_MAX_SRC == 8


# ---------------------------------------------------------------- 3. the kernel's address arithmetic
def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_concat_i8_geom.h holds the kernel's lane -> (sources, offsets, masks, loads) functions and compiles as host
    code: scripts/concat_geom_check.cpp walks every lane of every launch and exits non-zero on a load outside its source, an
    unaligned load, a byte that is not the byte the index rule names, an output chunk written twice or not at all, or an aligned
    launch that holds anything but 16-byte loads -- over its built-in list and over the GPU tests' shape list.  The list reaches
    each path (16-byte, aligned dwords, byte-shifted dwords, chunks of two or more sources) without and with an upsampled source."""
    exe = str(tmp_path / "concat_geom_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "concat_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
    out = subprocess.run([exe] + [nn_.case_arg(c) for c in nn_.KERNEL_CASES], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(nn_.KERNEL_CASES) + 1, out.stdout + out.stderr
    rows = nn_.class_rows(lines)
    nn_.check_paths_reached(rows)


# ---------------------------------------------------------------- 4. the cost script's byte accounting
def test_cost_script_accounts_the_closed_form_for_inception_224():
    """Per block with branch widths a, b, c, d on N x H x W pixels, p = pad16: nested launches move
    p(a) + p(b) + p(a+b)  +  p(a+b) + p(c) + p(a+b+c)  +  p(a+b+c) + p(d) + p(a+b+c+d) bytes per pixel, the flat one
    p(a) + p(b) + p(c) + p(d) + p(a+b+c+d).  The plans come from the model itself (planned at 32 x 32: the plan does not depend on
    the size), the shapes from a shape-only forward at 224 x 224 with 256 images."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import concat_flat_cost as cost
    finally:
        sys.path.pop(0)
    from common.quantity import resident
    from model.inception.Inception_fabu import LAYOUT
    p = cost.pad16
    shapes = cost.concat_shapes(an.inception(224), 256, 224)
    assert len(shapes) == 12
    with concat_n_doubles.installed():
        float_model = an.inception(32)
        x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
        bits = dn.measured_out_bits(copy.deepcopy(float_model), x)
        net = dn.rebuild(float_model, an.inception_info(float_model, bits)).eval()
        totals = {}
        for key in ("off", "on"):
            summary = resident.enable(net, x, verify=False, concat=True, avgpool=True, flatten=(key == "on"))
            assert summary["resident_concats"] == 12 and summary.get("flattened_concats", 0) == (8 if key == "on" else 0)
            rows = cost.concat_launch_bytes(resident.describe(net), shapes)
            assert len(rows) == (4 if key == "on" else 12)
            totals[key] = sum(b for _n, _l, b in rows)
    nested = flat = 0
    plane = 55
    for item in LAYOUT:
        if item[0] == "transition":
            plane //= 2
            continue
        a, b, c, d = item[0], item[2], item[4], item[5]
        pix = 256 * plane * plane
        nested += pix * (p(a) + p(b) + p(a + b) + p(a + b) + p(c) + p(a + b + c) + p(a + b + c) + p(d) + p(a + b + c + d))
        flat += pix * (p(a) + p(b) + p(c) + p(d) + p(a + b + c + d))
    assert totals == {"off": nested, "on": flat} and flat < nested, (totals, nested, flat)
    assert (nested, flat) == (NESTED_BYTES_224, FLAT_BYTES_224)                 # the two totals of DESIGN section 20


NESTED_BYTES_224, FLAT_BYTES_224 = 1677393920, 655073280
