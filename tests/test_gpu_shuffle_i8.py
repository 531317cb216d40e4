"""fq_shuffle_i8_nhwc on the MI355X against the index rule in numpy (tests/shuffle_nets.shuffle_rule), and the toy ShuffleNetV2 of
golden G20 and the full-width model end to end with resident.enable(shuffle=True).  Every comparison is exact.   pytest -m gpu

The kernel's shapes (shuffle_nets.KERNEL_CASES) are the smallest at which each mechanism can go wrong: groups == C, C / groups odd,
C below 16, C no multiple of 4, C a multiple of 16; slices at a byte offset (the right half of 116 and of 244 channels), at an
aligned offset, of one byte at the end of a row; a shuffled slice; 1, 3, tile - 1, tile + 1 and 2 * 7 * 9 pixels; and one shape
with one tile more than the capped grid has workgroups (2048 * 64 + 1 pixels of 16 bytes), so that the stride loop iterates.  The
input's padding channels hold non-zero junk, the output is pre-filled with 0x55 and lies inside a larger allocation whose bytes
in front of and behind it must stay as they were."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import depthwise_nets as dn
import shuffle_nets as sn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

GUARD = 256
ON = {"depthwise": True, "concat": True, "shuffle": True}


def _source(case, seed):
    """(x int8 [N, H, W, Cpad_in] on the host with non-zero junk in its padding channels, c_in)"""
    n, h, w, cpad_in, c_off, c, _g = case
    c_in = max(c_off + c, cpad_in - 15)                       # the smallest channel count stored as Cpad_in that holds the range
    rng = np.random.default_rng(seed)
    x = rng.integers(-128, 128, (n, h, w, cpad_in), dtype=np.int8)
    x[..., c_in:] = rng.integers(1, 128, (n, h, w, cpad_in - c_in), dtype=np.int8)
    return x, c_in


@pytest.mark.parametrize("case", sn.KERNEL_CASES, ids=sn.case_arg)
def test_kernel_matches_the_rule_and_writes_nothing_outside_its_output(case):
    from common.quantity import _native
    n, h, w, cpad_in, c_off, c, g = case
    x, c_in = _source(case, seed=sum(case))
    assert _native.shuffle_supported(c_in, c_off, c, g)
    want = sn.shuffle_rule(x, c_off, c, g)
    cpad = sn.pad16(c)
    nbytes = n * h * w * cpad
    arena = torch.full((GUARD + nbytes + GUARD,), 0x55, dtype=torch.int8, device="cuda")
    out = arena[GUARD:GUARD + nbytes].view(n, h, w, cpad)
    xd = torch.from_numpy(x).cuda()
    got = _native.shuffle_i8_nhwc(xd, c_in, c_off, c, g, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = arena.cpu().numpy()
    assert (host[:GUARD] == 0x55).all() and (host[GUARD + nbytes:] == 0x55).all()
    np.testing.assert_array_equal(host[GUARD:GUARD + nbytes].reshape(n, h, w, cpad), want)
    assert (want[..., c:] == 0).all()
    np.testing.assert_array_equal(xd.cpu().numpy(), x)                                  # the source is only read
    if g > 1 and c_off == 0 and c == c_in:                                              # ... and it is torch.channel_shuffle
        t = torch.channel_shuffle(torch.from_numpy(x[..., :c].astype(np.float32)).permute(0, 3, 1, 2), g).permute(0, 2, 3, 1)
        np.testing.assert_array_equal(want[..., :c], t.numpy().astype(np.int8))
    # a fresh output tensor gives the same bytes
    np.testing.assert_array_equal(_native.shuffle_i8_nhwc(xd, c_in, c_off, c, g).cpu().numpy(), want)


def test_the_call_with_nothing_to_do_and_a_range_outside_the_source_are_refused():
    from common.quantity import _native
    x = torch.zeros(1, 2, 2, 64, dtype=torch.int8, device="cuda")
    assert not _native.shuffle_supported(64, 0, 64, 1)
    with pytest.raises(_native.FqError):
        _native.shuffle_i8_nhwc(x, 64, 0, 64, 1)
    with pytest.raises(_native.FqError):
        _native.shuffle_i8_nhwc(x, 64, 20, 48, 1)
    with pytest.raises(_native.FqError):
        _native.shuffle_i8_nhwc(x, 64, 0, 60, 7)
    with pytest.raises(_native.FqError):
        _native.shuffle_i8_nhwc(x.cpu(), 64, 0, 64, 2)
    assert _native.shuffle_i8_nhwc(x[:0], 64, 0, 64, 2).shape == (0, 2, 2, 64)          # N == 0: FQ_OK, nothing launched


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def g20(golden_dir):
    with open(os.path.join(golden_dir, "g20_shuffle_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g20_shuffle_net.npz"))


def test_g20_logits_on_the_hip_kernels_with_the_switch_off_on_and_as_a_graph(g20, monkeypatch):
    from common.quantity import _native, resident
    ref, arrays = g20
    want = arrays["logits_recon"]
    x = sn.integer_input().cuda()
    net = dn.rebuild(sn.integer_weights(sn.g20_net()).eval(), copy.deepcopy(ref["quantity_information"])).cuda()
    launches = []
    real = _native.shuffle_i8_nhwc
    monkeypatch.setattr(_native, "shuffle_i8_nhwc", lambda *a, **k: (launches.append(a[1:]), real(*a, **k))[1])
    with torch.no_grad():
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)                      # fp32 module boundaries
        off = resident.enable(net, x, depthwise=True, concat=True)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)
        assert "resident_shuffles" not in off and off["resident_concats"] == 1 and off["fp32_outputs"] == 3 and not launches
        on = resident.enable(net, x, **ON)
        plans = resident.describe(net)
        del launches[:]
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)
        assert launches == [(20, 0, 20, 2), (20, 0, 10, 1), (20, 10, 10, 1), (20, 0, 20, 2), (20, 0, 10, 1), (20, 10, 10, 1),
                            (20, 0, 20, 2)]
        np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["resident_shuffles"] == 3 and on["resident_slices"] == 4 and on["resident_concats"] == 3
        assert on["fp32_outputs"] == 0 and not plans.shuffle_left
        graphed = resident.capture(net, x)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)
        np.testing.assert_array_equal(graphed(x).cpu().numpy(), want)                  # a second replay
        resident.disable(net)
        np.testing.assert_array_equal(net(x).cpu().numpy(), want)


def test_the_full_width_model_gives_the_same_logits_with_and_without_the_switch():
    """ShuffleNetV2 1.0x (116 / 232 / 464 / 1024: halves of 58, 116 and 232 channels) on 64 x 64 images without BatchNorm, seeded
    integer weights and fixed bits: every one of its 16 shuffles and 26 slices runs on the integers and no layer between the stem
    and conv5 writes fp32."""
    from common.quantity import resident
    x = sn.integer_input((2, 3, 64, 64))
    model = sn.integer_weights(sn.full_model(num_classes=10, width_mult=1.0, input_size=64, batch_norm=False)).eval()
    net = dn.rebuild(model, sn.unit_info(model, x)).cuda()
    x = x.cuda()
    with torch.no_grad():
        plain = net(x)
        off = resident.enable(net, x, depthwise=True, concat=True)
        assert torch.equal(net(x), plain)
        on = resident.enable(net, x, **ON)
        assert torch.equal(net(x), plain) and torch.equal(net(x[:1]), plain[:1])
    assert on["resident_shuffles"] == 16 and on["resident_slices"] == 26 and on["resident_concats"] == 16
    assert on["fp32_outputs"] == 0 and off["fp32_outputs"] > 0 and not resident.describe(net).shuffle_left
    assert float(plain.abs().max()) > 0


def test_calibration_on_the_gpu_writes_the_tables_of_the_reference(g20):
    """One GPU calibration of the G20 net on the shipped settings: the graph, the feat.table and the rewritten weight.table the
    reference wrote -- the ones the CPU oracle engine writes from the same activations (tests/test_shuffle_plan_cpu.py)."""
    from tools import Quantity
    ref, _arrays = g20
    shape = sn.G20_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="gpu", max_cali_img_num=2) as tmp:
        q = Quantity(sn.integer_weights(sn.g20_net()).eval().cuda())
        q.own_depthwise = True
        assert dict(q.net_info) == ref["net_info"] and list(q.net_info.keys()) == ref["net_info_order"]
        assert q.get_merge_groups(q.net_info) == ref["merge_groups"] and q.layers_num == ref["layers_num"]
        q.activation_quantize([(x.cuda(), y) for (x, y) in sn.integer_batches(3)])
        wd = os.path.join(tmp, "test", "workdir")
        assert open(os.path.join(wd, "feat.table")).read() == ref["feat_table"]
        q.weight_quantize()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table"]
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
