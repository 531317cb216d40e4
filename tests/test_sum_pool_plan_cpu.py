"""resident.enable(..., avgpool=True, sums=True) on a box without a GPU: a windowed nn.AvgPool2d reads the exact int16 sum of a
NewAdd -- the ResNet-D shortcut.  The tracer, the plan, the handles and the module glue run for real; the kernel entry points are
oracle-backed doubles (tests/sum_pool_doubles.py on top of avgpool_doubles.py) that follow the reference's fp32 chain literally.
Every comparison is exact.  The rule of include/fq.h (fq_avgpool_i16_nhwc) is held against torch's own chain on int16 sources, the
kernel's address arithmetic is walked on the host over the GPU tests' shape list (scripts/avgpool_i16_geom_check.cpp), golden G23
pins a calibrated toy ResNet-D to the reference, and forty random ResNet-D-shaped nets run under three plans."""
import io
import json
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import avgpool_nets as an
import cases
import sum_pool_doubles
import sum_pool_nets as sn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NINE = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
                sums=True)


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


class _Spy(object):
    """Counts the calls of the two pool entry points while installed."""

    def __init__(self, nat):
        self.nat, self.i8, self.i16 = nat, [], []

    def __enter__(self):
        self.real8, self.real16 = self.nat.avgpool_i8_nhwc, self.nat.avgpool_i16_nhwc
        self.nat.avgpool_i8_nhwc = lambda *a, **k: (self.i8.append(a[1:]), self.real8(*a, **k))[1]
        self.nat.avgpool_i16_nhwc = lambda *a, **k: (self.i16.append((a[0].dtype,) + a[1:]), self.real16(*a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.nat.avgpool_i8_nhwc, self.nat.avgpool_i16_nhwc = self.real8, self.real16


# ---------------------------------------------------------------- 1. the rule on int16 sources
def _torch_chain(x, C, kernel, stride, padding, cip, g, b, relu):
    """DeQuantity(g) -> nn.AvgPool2d -> nn.ReLU -> Quantity(b) with torch's CPU operators, on int16 NHWC."""
    f = torch.from_numpy(x[..., :C].astype(np.float32)).permute(0, 3, 1, 2).contiguous() * float(2.0 ** -g)
    y = nn.AvgPool2d(kernel, stride, padding, ceil_mode=False, count_include_pad=cip)(f)
    if relu:
        y = torch.relu(y)
    q = torch.clamp(torch.round(y * float(2.0 ** b)), -128, 127)
    out = np.zeros(tuple(q.shape[:1]) + tuple(q.shape[2:]) + (x.shape[-1],), np.int8)
    out[..., :C] = q.permute(0, 2, 3, 1).numpy().astype(np.int8)
    return out


@pytest.mark.parametrize("case", an.KERNEL_CASES, ids=an.case_arg)
def test_the_numpy_rule_is_torchs_chain_on_int16_sources(case):
    """|S| <= 64 * 32768 = 2^21 < 2^24: every partial sum of torch's fp32 accumulation and (float)S are exact, so the rule of the
    int8 pool holds word for word -- over what a sum on grid g can hold, both ends planted, planes of all-max and all-min, and
    the whole of int16."""
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    C, kernel, stride, padding = case[3], case[4:6], case[6:8], case[8:10]
    checked = 0
    for g in sn.GRIDS:
        for kind in ("grid", "max", "min", "random"):
            x = sn.source16(rng, case, kind, g)
            assert x.dtype == np.int16
            for cip in (False, True):
                for relu in (False, True):
                    for shift in sn.RULE_SHIFTS:
                        want = _torch_chain(x, C, kernel, stride, padding, cip, g, g + shift, relu)
                        got = an.numpy_rule(x, C, kernel, stride, padding, cip, shift, relu)
                        np.testing.assert_array_equal(got, want, err_msg=str((g, kind, cip, relu, shift)))
                        checked += got[..., :C].size
    assert checked > 0


def test_ties_round_half_to_even_on_every_grid_and_the_double_follows():
    with sum_pool_doubles.installed() as nat:
        for g in sn.GRIDS:
            x = sn.tie_source16(g)
            assert x.dtype == np.int16 and int(np.abs(x).max()) == 6 << g
            for shift, want in ((-g, [[0, 2, 2], [0, -2, -2], [1, 3, -1]]), (-g - 1, [[0, 1, 1], [0, -1, -1], [0, 2, 0]])):
                if shift < -8:
                    continue
                got = an.numpy_rule(x, 16, (2, 2), (2, 2), (0, 0), True, shift, False)
                assert got[0, :, :, 0].tolist() == want and (got == got[..., :1]).all()     # half away from zero: 1, 2, 3, -1, ...
                dbl = nat.avgpool_i16_nhwc(torch.from_numpy(x), 16, (2, 2), (2, 2), (0, 0), True, shift, False)
                np.testing.assert_array_equal(dbl.numpy(), got)
                np.testing.assert_array_equal(_torch_chain(x, 16, (2, 2), (2, 2), (0, 0), True, g, g + shift, False), got)


def test_the_double_is_the_rule_on_the_case_list():
    with sum_pool_doubles.installed() as nat:
        for case in an.KERNEL_CASES:
            rng = np.random.default_rng(23 + sum(case))
            x = sn.source16(rng, case)
            for cip, relu, shift in ((True, False, 0), (False, True, 1), (False, False, -8), (True, True, 8)):
                got = nat.avgpool_i16_nhwc(torch.from_numpy(x), case[3], case[4:6], case[6:8], case[8:10], cip, shift, relu)
                np.testing.assert_array_equal(got.numpy(), an.numpy_rule(x, case[3], case[4:6], case[6:8], case[8:10], cip, shift, relu))


def test_avgpool_i16_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.avgpool_i16_supported
    assert ok((3, 3), (1, 1), (1, 1), 0) and ok((2, 2), (2, 2), (0, 0), -8) and ok((8, 8), (8, 8), (4, 4), 8) and ok((1, 64), (1, 1), (0, 32), 0)
    assert not ok((9, 9), (1, 1), (4, 4), 0) and not ok((5, 13), (1, 1), (0, 0), 0) and not ok((65, 1), (1, 1), (0, 0), 0)
    assert not ok((3, 3), (1, 1), (1, 1), 9) and not ok((3, 3), (1, 1), (1, 1), -9)
    assert not ok((3, 3), (1, 1), (2, 1), 0) and not ok((3, 3), (1, 1), (-1, 0), 0) and not ok((0, 3), (1, 1), (0, 0), 0)
    assert not ok((3, 3), (0, 1), (0, 0), 0) and not ok((65536, 65536), (1, 1), (0, 0), 0)


# ---------------------------------------------------------------- 2. what is planned
def test_the_pool_behind_a_sum_is_declined_without_sums_and_planned_with_it():
    """avgpool_nets.PoolNet(mode="add_source"): with avgpool=True alone the parent's plan (the add writes fp32 for the pool); with
    sums=True the add goes from emit_f32 to integer-only with want_wide, and the pool runs on the int16 entry point."""
    from common.quantity import resident
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = an.PoolNet(mode="add_source").eval(), an.example()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.abs().max()) > 0
        off = resident.enable(net, x, avgpool=True)
        rows = _rows(net)
        assert resident.enable(net, x, avgpool=True, sums=False) == off and rows == _rows(net)
        plans = _plans(net)
        assert off["resident_avgpools"] == 0 and "resident_sum_avgpools" not in off and "pool" not in plans
        assert plans["add"].emit_f32 and plans["add"].want_wide and not plans.avgpool_left
        _check_forwards(net, x, plain)
        assert not spy.i8 and not spy.i16

        on = resident.enable(net, x, avgpool=True, sums=True)                  # verify=True
        plans = _plans(net)
        assert on["resident_avgpools"] == 1 and on["resident_sum_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] - 1
        assert set(on) == set(off) | {"resident_sum_avgpools"} and not plans.avgpool_left
        add, pool = plans["add"], plans["pool"]
        assert not add.emit_f32 and add.emit_int and add.want_wide and add.narrow_bit is None and add.relu and add.grid == 4
        assert pool.emit_int and not pool.emit_f32 and pool.grid == 4 and pool.narrow_bit == 4 and not pool.relu
        assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolWindowResident)
        spy.i16[:] = []
        _check_forwards(net, x, plain)
        assert len(spy.i16) == 3 and not spy.i8
        assert spy.i16[0] == (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, 0, False)
        # the add hands out the exact int16 sum and nothing else; the pool's handle carries the narrow payload only
        with torch.no_grad():
            s = net.r0(net.stem(x))
            t = net.radd(net.add(net.a(s), net.b(s)))
            h = net.pool(t)
        assert type(t) is resident.QHandle and t.exact.dtype == torch.int16 and t.narrow is None and t.relu_done and t.grid == 4
        assert type(h) is resident.QHandle and h.exact is None and h.narrow.dtype == torch.int8 and h.bit == 4 and h.relu_done
        assert tuple(h.shape) == (4, 16, 6, 6)
        with pytest.raises(nat.FqError):
            h.to_f32()
        resident.disable(net)
        assert not _plans(net) and not _plans(net).avgpool_left and all("forward" not in m.__dict__ for m in net.modules())
        assert "avgpool_left" not in net.__dict__.get("_fq_resident_report", {})
        spy.i16[:] = []
        _check_forwards(net, x, plain)
        assert not spy.i16


# what the fusion passes make of a ResNet-D block (decided from the code, held here either way):
#   identity  the front's add runs its conv3 (fused_conv_adds) and writes wide + narrow: conv1 reads narrow, the pool wide
#   skip      ... and a later add reads the same wide tensor: two exact readers and one narrow reader
#   tail      the second front add is fq_block_tail_i8 (its conv3 + add + the D block's conv1): the pool reads the wide tensor
#             that launch wrote; the narrow form stays in LDS (narrow_to_hbm False: conv1 is its only reader)
#   proj      fq_block_tail_proj_i8 takes conv3 + add + projection with the POOLED tensor as the projection's operand at stride 1
#             (_newadd_fused_conv_proj_add takes the projection's xq and stride separately)
D_NETS = {
    "identity": (lambda: sn.DBlockNet(), "f1.add", dict(fused_block_tails=0, fused_projections=0)),
    "skip": (lambda: sn.DBlockNet(skip=True), "f1.add", dict(fused_block_tails=0, fused_projections=0)),
    "tail": (lambda: sn.DBlockNet(front="tail"), "f2.add", dict(fused_block_tails=2, fused_projections=0)),
    "proj": (lambda: sn.DBlockNet(front="proj"), "f1.add", dict(fused_block_tails=0, fused_projections=1)),
    "pool_3x3": (lambda: sn.DBlockNet(pool=nn.AvgPool2d(3, 2, 1, count_include_pad=False)), "f1.add", dict(fused_projections=0)),
}


@pytest.mark.parametrize("tag", sorted(D_NETS))
def test_resnet_d_blocks(tag):
    from common.quantity import resident
    make, src, fusions = D_NETS[tag]
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = make().eval(), sn.example()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.abs().max()) > 0
        off = resident.enable(net, x, avgpool=True)
        assert _plans(net)[src].emit_f32 and "d.pool" not in _plans(net) and off["resident_avgpools"] == 0
        _check_forwards(net, x, plain)
        on = resident.enable(net, x, avgpool=True, sums=True)
        plans = _plans(net)
        assert on["resident_sum_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] - 1, (off, on)
        assert {k: on[k] for k in fusions} == fusions, on
        add = plans[src]
        assert not add.emit_f32 and add.want_wide and add.narrow_bit == 4 and add.relu and add.fuse_arg is not None
        assert plans["d.pool"].grid == 4 and plans["d.pool"].narrow_bit == 4
        if tag == "tail":
            assert add.fuse_next is net.d.conv1 and not add.narrow_to_hbm
        if tag == "proj":
            assert plans["d.add"].fuse_proj and plans["d.proj"].defer and off["fused_projections"] == 1
        if tag == "skip":
            assert plans["add2"].resident_add and not plans["add2"].emit_f32
        spy.i16[:] = []
        _check_forwards(net, x, plain)
        assert len(spy.i16) == 3 and not spy.i8
        assert spy.i16[0][2:5] == ((3, 3), (1, 1), (1, 1)) if tag == "skip" else True
        with torch.no_grad():                                                   # the sum the pool reads: wide and narrow, no fp32
            t = net.f1(net.r0(net.stem(x)))
            t = net.f2(t) if net.f2 is not None else t
        assert type(t) is resident.QHandle and t.exact.dtype == torch.int16
        assert (t.narrow is None) == (tag == "tail")
        if tag == "tail":
            assert t.next_out is not None and t.next_out[0] is net.d.conv1


SUM_NETS = {
    "relu_behind": (lambda: sn.SumPoolNet(relu_front=False, relu_behind=True), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, 0, True)),
    "relu_on_both_sides": (lambda: sn.SumPoolNet(relu_behind=True), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, 0, True)),
    "two_readers": (lambda: sn.SumPoolNet(pool=nn.AvgPool2d(3, 1, 1, count_include_pad=False), read_bits=(4, 4)),
                    (torch.int16, 16, (3, 3), (1, 1), (1, 1), False, 0, False)),
    "reader_at_another_bit": (lambda: sn.SumPoolNet(read_bits=(2,)), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, -2, False)),
    "operands_on_two_grids": (lambda: sn.SumPoolNet(sum_bits=(3, 6), read_bits=(5,)), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, -1, False)),
    "shift_8": (lambda: sn.SumPoolNet(sum_bits=(-1, -1), read_bits=(8,)), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, 8, False)),
    "shift_minus_8": (lambda: sn.SumPoolNet(sum_bits=(8, 8), read_bits=(0,)), (torch.int16, 16, (2, 2), (2, 2), (0, 0), True, -8, False)),
}


@pytest.mark.parametrize("tag", sorted(SUM_NETS))
def test_pools_behind_one_sum(tag):
    from common.quantity import resident
    make, call = SUM_NETS[tag]
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = make().eval(), sn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, avgpool=True)
        assert _plans(net)["add"].emit_f32
        on = resident.enable(net, x, avgpool=True, sums=True)
        plans = _plans(net)
        assert on["resident_sum_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] - 1 and not plans.avgpool_left
        assert not plans["add"].emit_f32 and plans["add"].want_wide and plans["add"].relu == net.relu_front
        assert plans["pool"].relu == net.relu_behind
        if net.relu_behind:
            assert isinstance(net.r1.__dict__["forward"], resident._ReluPassThrough)
        spy.i16[:] = []
        _check_forwards(net, x, plain)
        assert len(spy.i16) == 3 and spy.i16[0] == call and not spy.i8


DECLINED = {
    "two_bits": (lambda: sn.SumPoolNet(read_bits=(4, 3)), "different bits [3, 4]"),
    "shift_9": (lambda: sn.SumPoolNet(sum_bits=(-1, -1), read_bits=(9,)), "= 9: not taken by the kernel"),
    "shift_minus_9": (lambda: sn.SumPoolNet(sum_bits=(8, 8), read_bits=(-1,)), "= -9: not taken by the kernel"),
    "window_9x9": (lambda: sn.SumPoolNet(pool=nn.AvgPool2d(9, 1, 4)), "window 9x9"),
    "ceil_mode": (lambda: sn.SumPoolNet(pool=nn.AvgPool2d(2, ceil_mode=True)), "ceil_mode=True"),
    "divisor_override": (lambda: sn.SumPoolNet(pool=nn.AvgPool2d(2, divisor_override=3)), "divisor_override"),
    "called_twice": (lambda: sn.SumPoolNet(mode="twice"), "called more than once"),
    "concat_reader": (lambda: sn.SumPoolNet(mode="concat"), "read as fp32 by cat"),
    "foreign_reader": (lambda: sn.SumPoolNet(mode="foreign"), "code outside the plan"),
}


@pytest.mark.parametrize("tag", sorted(DECLINED))
def test_what_the_plan_declines_keeps_the_fp32_form_and_says_why(tag):
    from common.quantity import resident
    make, why = DECLINED[tag]
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = make().eval(), sn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, concat=True, avgpool=True)
        rows = _rows(net)
        on = resident.enable(net, x, concat=True, avgpool=True, sums=True)
        plans = _plans(net)
        assert on["resident_sum_avgpools"] == 0 and "forward" not in net.pool.__dict__, (on, plans)
        assert rows == _rows(net) and {k: v for k, v in on.items() if k != "resident_sum_avgpools"} == off
        assert plans["add"].emit_f32 and set(plans.avgpool_left) == {"pool"} and why in plans.avgpool_left["pool"], plans.avgpool_left
        _check_forwards(net, x, plain)
        assert not spy.i16 and not spy.i8


def test_avgpool_left_also_names_pools_without_an_integer_source():
    """The report covers every hooked windowed pool, not only those behind a sum: one behind a foreign tensor, one declined behind
    an int8 source; a planned one and the whole-plane pool are not in it."""
    from common.quantity import resident

    class Net(nn.Module):
        def __init__(self):
            from common.quantity import View
            super(Net, self).__init__()
            self.stem, self.r0 = sn.conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
            self.p_plain, self.p_ok, self.p_big = nn.AvgPool2d(2), nn.AvgPool2d(2), nn.AvgPool2d(9, 1, 4)
            self.c0, self.c1, self.c2 = sn.conv(16, 8, 1, 4, 4), sn.conv(16, 8, 1, 4, 4, seed=1), sn.conv(16, 8, 1, 4, 4, seed=2)
            self.gpool, self.view = nn.AvgPool2d(6), View()

        def forward(self, x):
            s = self.r0(self.stem(x))
            return self.c0(self.p_plain(s * 1.0)), self.view(self.gpool(self.c1(self.p_ok(s)))), self.c2(self.p_big(s))

    with sum_pool_doubles.installed():
        net, x = Net().eval(), sn.example()
        with torch.no_grad():
            plain = net(x)
        on = resident.enable(net, x, avgpool=True, sums=True)
        left = _plans(net).avgpool_left
        assert set(left) == {"p_plain", "p_big"} and on["resident_avgpools"] == 1 and on["resident_sum_avgpools"] == 0, left
        assert "no integer source" in left["p_plain"] and "window 9x9" in left["p_big"]
        _check_forwards(net, x, plain)
        resident.enable(net, x, avgpool=True)
        assert not _plans(net).avgpool_left                                     # filled only with sums=True


def test_sums_needs_avgpool():
    from common.quantity import resident
    with sum_pool_doubles.installed():
        net, x = sn.SumPoolNet().eval(), sn.example()
        for kw in (dict(sums=True), dict(sums=True, avgpool=False), dict(sums=True, concat=True)):
            with pytest.raises(ValueError, match="avgpool=True"):
                resident.enable(net, x, **kw)
        assert not resident.is_enabled(net) or not _plans(net).avgpool_left


def test_the_default_call_is_the_parents():
    """enable(net, x), enable(net, x, sums=False) and enable(net, x, avgpool=True): no new summary key, the same rows, no report."""
    from common.quantity import resident
    with sum_pool_doubles.installed():
        for make in (sn.SumPoolNet, sn.DBlockNet, lambda: an.PoolNet(mode="add_source")):
            net, x = make().eval(), sn.example()
            a = resident.enable(net, x)
            rows = _rows(net)
            b = resident.enable(net, x, sums=False)
            assert a == b and rows == _rows(net) and set(a) == an.DEFAULT_KEYS
            c = resident.enable(net, x, avgpool=True)
            assert set(c) == an.DEFAULT_KEYS | {"resident_avgpools"} and rows == _rows(net)
            assert not _plans(net).avgpool_left and "avgpool_left" not in net.__dict__.get("_fq_resident_report", {})
            assert set(resident.Plan.__slots__) == set(next(iter(_plans(net).values())).__slots__)
    # no field was added to Plan: a plan pickled before this change loads as it is
    assert resident.Plan.__slots__ == ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg",
                                       "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip", "perm", "table")


def test_the_forward_stays_adaptive():
    """A planned pool that meets an input it was not planned for falls back to torch on fp32."""
    from common.quantity import resident
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = sn.SumPoolNet().eval(), sn.example()
        resident.enable(net, x, avgpool=True, sums=True)
        with torch.no_grad():
            s = net.r0(net.stem(x))
            t = net.radd(net.add(net.a(s), net.b(s)))
            assert type(t) is resident.QHandle and t.exact.dtype == torch.int16
            f = t.to_f32()
            want = nn.functional.avg_pool2d(f, 2)
            spy.i16[:] = []
            assert torch.equal(net.pool(f), want) and not spy.i16                      # an fp32 tensor without a handle
            other = resident.QHandle(t.shape, t.exact, t.grid + 1, t.narrow, t.bit, t.relu_done)
            assert torch.equal(net.pool(other), nn.functional.avg_pool2d(other.to_f32(), 2)) and not spy.i16        # another grid
            net.pool.kernel_size, net.pool.stride, net.pool.padding = 9, 1, 4           # a window the kernel declines
            assert torch.equal(net.pool(t), nn.functional.avg_pool2d(f, 9, 1, 4)) and not spy.i16
            net.pool.kernel_size, net.pool.stride, net.pool.padding = 2, 2, 0
            assert type(net.pool(t)) is resident.QHandle and len(spy.i16) == 1 and not spy.i8
            i8 = resident.QHandle.int8(s.exact, 16, 4, True)                            # an int8 source on the planned grid: the int8 kernel
            assert type(net.pool(i8)) is resident.QHandle and len(spy.i8) == 1 and len(spy.i16) == 1
            plan = net.pool.__dict__.pop("_resident")
            assert torch.equal(net.pool(t), want) and len(spy.i16) == 1                 # no plan
            net.pool.__dict__["_resident"] = plan


def test_a_planned_model_pickles_with_its_plan_and_disable_removes_it():
    from common.quantity import resident
    with sum_pool_doubles.installed():
        for make, pool in ((sn.SumPoolNet, "pool"), (sn.DBlockNet, "d.pool"), (lambda: sn.DBlockNet(front="tail"), "d.pool")):
            net, x = make().eval(), sn.example()
            with torch.no_grad():
                plain = net(x)
            resident.enable(net, x, avgpool=True, sums=True)
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert _rows(again).keys() == _rows(net).keys() and resident.is_enabled(again)
            assert isinstance(again.get_submodule(pool).__dict__["forward"], resident._AvgPoolWindowResident)
            assert _plans(again).avgpool_left == _plans(net).avgpool_left == {}
            with torch.no_grad():
                assert _same(again(x), plain)
            resident.disable(again)
            assert not _plans(again) and "forward" not in again.get_submodule(pool).__dict__
            assert not any(k.startswith("_fq_resident") for k in again.__dict__)
            with torch.no_grad():
                assert _same(again(x), plain)


def test_a_plan_pickled_before_this_change_still_loads():
    """The state of a Plan written by the parent: exactly today's fields (none was added), restored by __setstate__."""
    from common.quantity import resident
    old = dict(relu=True, emit_f32=False, emit_int=True, narrow_bit=4, want_wide=True, grid=4, resident_add=True, defer=False, fuse_arg=0,
               fuse_next=None, narrow_to_hbm=True, fuse_proj=False, depthwise=False, up=None, grouped=False, clip=False, perm=None, table=None)
    p = resident.Plan()
    p.__setstate__(old)
    assert p.__getstate__() == old
    q = pickle.loads(pickle.dumps(p))
    assert q.__getstate__() == old and q.sum_outputs() == (True, True)


# ---------------------------------------------------------------- 3. the walker
def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_avgpool_i16_geom.h holds the kernel's lane -> (item, taps, divisor, byte offsets, mask) functions and compiles as host
    code: scripts/avgpool_i16_geom_check.cpp walks every lane of every launch and exits non-zero on a load outside the source, an
    unaligned load, a tap that is not in window ∩ image or is loaded twice, a wrong divisor or mask, or an output byte written twice
    or not at all -- over its built-in list and over the GPU tests' shape list."""
    exe = str(tmp_path / "avgpool_i16_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "avgpool_i16_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
    shapes = an.KERNEL_CASES + [sn.STRIDE_LOOP_CASE, (1, 6, 6, 16, 2, 2, 2, 2, 0, 0)]
    out = subprocess.run([exe] + [an.case_arg(c) for c in shapes], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(shapes) + 1, out.stdout + out.stderr
    stride_loop = [ln for ln in lines if ln.startswith("case " + an.case_arg(sn.STRIDE_LOOP_CASE))][0].split()
    assert int(stride_loop[stride_loop.index("items") + 1]) > 2048 * 256 and int(stride_loop[stride_loop.index("blocks") + 1]) == 2048
    # the smallest square plane of this family for 8 channels per lane: one row and column less gives every lane exactly one item
    n, h, w, c = sn.STRIDE_LOOP_CASE[:4]
    assert n * h * w * c // 8 > 2048 * 256 >= n * (h - 1) * (w - 1) * c // 8
    bad = subprocess.run([exe, "1,4,4,16,9,9,1,1,4,4"], capture_output=True, text=True)     # 81 taps: not a case the entry point launches
    assert bad.returncode == 1


# ---------------------------------------------------------------- 4. golden G23: a calibrated toy ResNet-D
@pytest.fixture(scope="module")
def g23(golden_dir):
    with open(os.path.join(golden_dir, "g23_resnetd_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g23_resnetd_net.npz"))


def test_g23_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g23, oracle):
    """The reference's graph discovery, merge groups, feat.table, weight.table and quantity information of sum_pool_nets.g23_net
    byte for byte through the oracle-backed CPU engine, and its ReconModel logits bit for bit: plain, with avgpool=True and with
    avgpool=True, sums=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g23
    shape = sn.G23_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(sn.g23_net(), base_seed=sn.G23_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(cases.calib_batches(3, shape, seed=sn.G23_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(sn.g23_net(), base_seed=sn.G23_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        # the convolution behind each pool reads at the Eltwise's bit, as after any pruned one-input op
        table = dict((ln.split()[0], ln.split()[1:]) for ln in ref["feat_table"].splitlines() if ln.strip())
        assert info["block2.downsample.1"]["input_bit"] == int(table["block1.Eltwise"][0]) == info["block2.conv1"]["input_bit"]
        assert info["block3.downsample.1"]["input_bit"] == int(table["block2.Eltwise"][0]) == info["block3.conv1"]["input_bit"]
        with sum_pool_doubles.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = cases.fixed_input(shape, seed=sn.G23_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x, avgpool=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off_plans = _plans(net)
                on = resident.enable(net, x, avgpool=True, sums=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            plans = _plans(net)
            assert off["resident_avgpools"] == 0 and on["resident_avgpools"] == on["resident_sum_avgpools"] == 2, (off, on)
            assert off["fp32_outputs"] - on["fp32_outputs"] == 2 and not plans.avgpool_left
            for name in ("block1.Eltwise", "block2.Eltwise"):
                assert off_plans[name].emit_f32 and not plans[name].emit_f32 and plans[name].want_wide and plans[name].narrow_bit is not None
            assert isinstance(net.pool_g.__dict__["forward"], resident._AvgPoolResident) and "pool_g" not in plans
            assert isinstance(net.block2.downsample[0].__dict__["forward"], resident._AvgPoolWindowResident)


# ---------------------------------------------------------------- 5. the random family
SEEDS = list(range(40))


def test_the_random_family_has_a_pool_over_a_sum_in_every_model_and_three_quarters_admitted():
    """By construction (no plan needed): every model has at least one pool over a sum; 51 of the 60 pools of the forty models are
    in the class the rule admits (one reader bit, |b - g| <= 8), 9 have readers at two bits."""
    pools = [p for seed in SEEDS for p in sn.RandomResNetD(seed).pools]
    assert all(len(sn.RandomResNetD(seed).pools) >= 1 for seed in SEEDS)
    admitted = sum(1 for _n, ok in pools if ok)
    print("random family: %d pools over a sum, %d admitted" % (len(pools), admitted))
    assert (len(pools), admitted) == (60, 51) and 4 * admitted >= 3 * len(pools)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_resnet_d(seed):
    """Each drawn model under the plans `avgpool`, `avgpool + sums` and all nine switches: exact logits, and with `sums` every pool
    the rule admits is planned (a condition, not a measurement), every other one is named in avgpool_left."""
    from common.quantity import resident
    with sum_pool_doubles.installed_all():
        net = sn.RandomResNetD(seed).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        want = sum(1 for _n, ok in net.pools if ok)
        a = resident.enable(net, x, avgpool=True)
        assert a["resident_avgpools"] == 0
        _check_forwards(net, x, plain)
        for kw in (dict(avgpool=True, sums=True), ALL_NINE):
            on = resident.enable(net, x, **kw)
            plans = _plans(net)
            assert on["resident_sum_avgpools"] == want == on["resident_avgpools"], (on, net.pools, plans.avgpool_left)
            for name, ok in net.pools:
                assert (name in plans) == ok and (name in plans.avgpool_left) == (not ok), (name, plans.avgpool_left)
                g, b = (plans[name].grid, plans[name].narrow_bit) if ok else (0, 0)
                assert abs(b - g) <= 8
            assert on["fp32_outputs"] == a["fp32_outputs"] - want
            _check_forwards(net, x, plain)
        resident.disable(net)
        _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 6. the model file
def test_resnet_d_needs_a_multiple_of_32():
    from model.resnetd.ResNetD_fabu import ResNet50D, ResNet101D
    for size in (0, 16, 48, 225):
        with pytest.raises(ValueError):
            ResNet50D(10, size)
    net = ResNet101D(10, 64)
    assert len(net.layer3) == 23 and sum(isinstance(m, nn.AvgPool2d) for m in net.modules()) == 4     # three shortcuts and the head's


# ---------------------------------------------------------------- 7. a window that is the whole plane
def test_a_whole_plane_pool_over_a_sum_in_front_of_a_convolution_takes_the_window_kernel():
    """The last shortcut of a ResNet-D at a small input: AvgPool2d(2, 2) on a 2 x 2 plane.  Without `sums` the whole-plane path
    reads the sum's exact integers and hands fp32 to the projection (the parent's plan); with it the pool runs on the int16
    window kernel and hands int8.  A whole plane of more than 64 taps keeps the whole-plane path and is not reported."""
    from common.quantity import resident
    with sum_pool_doubles.installed() as nat, _Spy(nat) as spy:
        net, x = sn.SumPoolNet(pool=nn.AvgPool2d(6)).eval(), sn.example(size=6)
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, avgpool=True)
        assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolResident) and off["resident_pools"] == 1
        assert not _plans(net)["add"].emit_f32 and "pool" not in _plans(net)
        _check_forwards(net, x, plain)
        assert not spy.i16
        on = resident.enable(net, x, avgpool=True, sums=True)
        plans = _plans(net)
        assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolWindowResident) and on["resident_pools"] == 0
        assert on["resident_sum_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] and not plans.avgpool_left
        assert not plans["add"].emit_f32 and plans["add"].want_wide and plans["pool"].narrow_bit == 4
        spy.i16[:] = []
        _check_forwards(net, x, plain)
        assert len(spy.i16) == 3 and spy.i16[0][2:5] == ((6, 6), (6, 6), (0, 0))

        big, xb = sn.SumPoolNet(pool=nn.AvgPool2d(12)).eval(), sn.example()         # 144 taps: not the window kernel's
        with torch.no_grad():
            plain = big(xb)
        on = resident.enable(big, xb, avgpool=True, sums=True)
        assert isinstance(big.pool.__dict__["forward"], resident._AvgPoolResident) and on["resident_pools"] == 1
        assert on["resident_sum_avgpools"] == 0 and not _plans(big).avgpool_left and not _plans(big)["add"].emit_f32
        _check_forwards(big, xb, plain)
