"""nn.ConvTranspose2d in graph discovery, the tables, ReconModel and the resident integer plan, on a box without a GPU (DESIGN
section 35): golden G28 (tests/golden/make_golden_deconv.py) on the oracle-backed engine, NewConvTranspose2d and
resident.enable(deconv=True) on oracle-backed doubles (tests/deconv_doubles.py: torch's float64 conv_transpose2d + the oracle's
tail, held against the kernel's phase-by-phase form), what the plan leaves in fp32 form and why, the host arithmetic of
fq_deconv2d_i8_resident, and the kernel's guards and address arithmetic walked on the host (scripts/deconv_geom_check.cpp).  Every
comparison is exact."""
import copy
import ctypes
import io
import json
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import activation_nets as an
import deconv_doubles as dd
import deconv_nets as dn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals are tried where a guard that fails cannot launch: no GPU")
INVALID, UNSUPPORTED = -1, -4
ALL14 = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
             sums=True, topdown=True, bilinear=True, requant=True, pixelshuffle=True, deconv=True)


@pytest.fixture(scope="module")
def g28(golden_dir):
    with open(os.path.join(golden_dir, "g28_deconv_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g28_deconv_net.npz"))


def _rows(plans):
    return sorted((n, p.emit_f32, p.emit_int, p.relu) for n, p in plans.items())


# ---------------------------------------------------------------- 1. the switch, the settings, the header, the model
def test_the_switch_is_accepted_and_off_by_default():
    """On the parent enable(deconv=True) is a TypeError."""
    import inspect
    from common.quantity import resident
    sig = inspect.signature(resident.enable)
    assert sig.parameters["deconv"].default is False and len([p for p in sig.parameters.values() if p.default is False]) == 14
    with dd.installed():
        net = dn.ToyNet("conv_dc_conv").eval()
        on = resident.enable(net, dn.example(), deconv=True)
        assert on["resident_deconvs"] == 1 and list(on)[-1] == "fused_projections"
        off = resident.enable(net, dn.example())
        assert "resident_deconvs" not in off and resident.describe(net).deconv_left == {}
        with pytest.raises(TypeError):
            resident.enable(net, dn.example(), deconvs=True)


def test_the_settings_the_header_and_the_bindings_name_the_feature():
    import yaml
    import common.quantity as cq
    from common.quantity import _native, new_quantity_op, resident
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        text = fh.read()
    settings = yaml.safe_load(text)["SETTINGS"]
    assert settings["CARE_OP_TYPE"][-1] == "ConvTranspose2d" and settings["ALL_OP_TYPE"][-1] == "ConvTranspose2d" and "G28" in text
    assert "ConvTranspose2d" not in settings["ALLOW_SAME_TID_OP_TYPE"] and "ConvTranspose2d" not in settings["MERGE_OP_YTPE"]
    header = open(os.path.join(ROOT, "include", "fq.h")).read()
    assert re.search(r"^int fq_deconv2d_i8_supported\(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h, "
                     r"int pad_w, int outpad_h,\s+int outpad_w, int dil_h, int dil_w, int rs_min, int rs_max\);", header, re.M)
    assert re.search(r"^int fq_deconv2d_i8_resident\(const int8_t\* x_nhwc, const int8_t\* w_pack, const float\* qbias, int8_t\* q_nhwc, "
                     r"int Cpad, int Kpad,\s+int relu, int N, int H, int W, int C, int K, int R, int S, int stride_h, int stride_w, "
                     r"int pad_h,\s+int pad_w, int outpad_h, int outpad_w, int rs, int ob, fq_stream_t stream\);", header, re.M)
    assert re.search(r"^int fq_deconv2d_i8_resident_act\(", header, re.M) and re.search(r"^size_t fq_deconv2d_i8_packed_bytes\(", header, re.M)
    assert "fq_deconv2d_i8_resident_pcs" not in header
    assert re.search(r"#define\s+FQ_VERSION\s+103\b", header) and _native.lib().fq_version() == 103
    L = _native.lib()
    assert len(L.fq_deconv2d_i8_supported.argtypes) == 15 and len(L.fq_deconv2d_i8_resident.argtypes) == 23
    assert len(L.fq_deconv2d_i8_resident_act.argtypes) == 24 and L.fq_deconv2d_i8_packed_bytes.restype is ctypes.c_size_t
    assert callable(_native.deconv_supported) and callable(_native.pack_weight_deconv) and callable(_native.deconv2d_i8_resident)
    assert _native.CONV_VARIANTS[16] == "deconv"
    assert cq.NewConvTranspose2d is new_quantity_op.NewConvTranspose2d and "NewConvTranspose2d" in cq.__all__
    assert "_w_dc" in new_quantity_op._WEIGHT_SLOTS and new_quantity_op.NewConvTranspose2d.use_deconv_i8 is False
    assert resident.Plan.__slots__ == ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer",
                                       "fuse_arg", "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip",
                                       "perm", "table")
    assert resident._SWITCH_TABLE[-1] == ("deconv", ("resident_deconvs",), ("deconv_left",)) and len(resident._SWITCH_TABLE) == 14
    makefile = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "Makefile")).read()
    assert "fq_deconv_i8.hip" in makefile and "fq_deconv_i8_geom.h" in makefile


def test_unet_takes_the_up_convolutions_and_keeps_its_default():
    for k, geometry in ((2, (2, 2, 0, 0)), (3, (3, 2, 1, 1)), (4, (4, 2, 1, 0))):
        m = dn.unet_model(input_size=32, base_width=8, depth=2, up="deconv", up_kernel=k).eval()
        ups = [mod for mod in m.modules() if isinstance(mod, nn.ConvTranspose2d)]
        assert [(u.in_channels, u.out_channels) for u in ups] == [(32, 16), (16, 8)]
        assert all((u.kernel_size[0], u.stride[0], u.padding[0], u.output_padding[0]) == geometry for u in ups)
        assert not any(isinstance(mod, nn.Upsample) for mod in m.modules())
        with torch.no_grad():
            assert m(torch.zeros(1, 3, 32, 32)).shape == (1, 2, 32, 32)
    for bad in (5, 1, 0, "2", True, None):
        with pytest.raises(ValueError):
            dn.unet_model(up="deconv", up_kernel=bad)
    with pytest.raises(ValueError):
        dn.unet_model(up="nearest")
    plain = dn.unet_model(input_size=32, base_width=8, depth=2)
    keys = list(plain.state_dict().keys())
    assert len(keys) == 62 and not any(k.startswith("ups.") for k in keys) and all(isinstance(u, nn.Upsample) for u in plain.ups)
    assert [tuple(v.shape) for v in plain.state_dict().values()] == [tuple(v.shape) for v in dn.unet_model(
        input_size=32, base_width=8, depth=2, up="bilinear", up_kernel=4).state_dict().values()]
    assert plain.downs[1][0].out_channels == 16 and plain.decs[0][0].in_channels == 32 and plain.decs[0][0].out_channels == 8


# ---------------------------------------------------------------- 2. the rule, the pack, the kernel's double
def test_the_phase_form_is_the_rule_and_torchs_float64_transposed_convolution():
    """The NumPy double of the kernel (deconv_nets.phase_acc over the pack) against include/fq.h's rule written out, against float64
    F.conv_transpose2d, and both tails against each other, over the GPU cases."""
    from common.quantity import _native
    from oracle import fq_oracle
    fq_oracle.build()
    sat_lo = sat_hi = False
    for k, c in enumerate(dn.kernel_cases()):
        x, w, qb = dn.operands(np.random.default_rng(100 + k), c)
        acc = dn.f64_acc(x, w, c)
        assert np.array_equal(dn.rule_acc(x, w, c), acc), dn.case_id(c)
        pack = _native.pack_weight_deconv(torch.from_numpy(w.astype(np.float32)), c["stride"], c["pad"]).numpy()
        assert np.array_equal(pack, dn.pack_rule(w, c)) and np.array_equal(dn.unpack_rule(pack, c), w)
        assert pack.size == _native.lib().fq_deconv2d_i8_packed_bytes(c["C"], c["K"], *c["kernel"])
        assert np.array_equal(dn.phase_acc(x, pack, c), acc), dn.case_id(c)
        want = dn.oracle_tail(acc, qb, c)
        assert np.array_equal(dn.int_tail(acc.astype(np.int64), qb, c), want), dn.case_id(c)
        lo, hi = c["clip"] if c["clip"] else ((0, 127) if c["relu"] else (-128, 127))
        sat_lo, sat_hi = sat_lo or bool((want[..., :c["K"]] == lo).any()), sat_hi or bool((want[..., :c["K"]] == hi).any())
    assert sat_lo and sat_hi
    c = dn.case(1, 3, 3, 3, 2, (2, 2), (4, 4), (0, 0), (3, 3))                      # kernel < stride: most outputs are tail(0, bias)
    x, w, qb = dn.operands(np.random.default_rng(1), c)
    acc = dn.rule_acc(x, w, c)
    assert acc.shape == (1, 13, 13, 2) and not acc[:, 2::4].any() and not acc[:, 3::4].any() and not acc[:, 12].any() and acc.any()


# ---------------------------------------------------------------- 3. host arithmetic only
def test_supported_answers_on_both_sides_of_its_limits():
    from common.quantity import _native
    s = _native.deconv_supported

    def ok(C=8, K=8, groups=1, k=(2, 2), stride=(2, 2), pad=(0, 0), op=(0, 0), dil=(1, 1), rs=7):
        return s(C, K, groups, k[0], k[1], stride, pad, op, dil, rs)

    assert ok() and ok(C=1, K=1, k=(1, 1), stride=(1, 1), rs=1) and ok(k=(8, 8), stride=(4, 4), pad=(7, 7), op=(3, 3), rs=16)
    assert ok(k=(3, 3), pad=(1, 1), op=(1, 1)) and ok(k=(4, 4), pad=(1, 1)) and ok(k=(2, 3), stride=(2, 1)) and ok(k=(2, 2), stride=(4, 4))
    assert not ok(groups=2) and not ok(dil=(2, 1)) and not ok(dil=(1, 2)) and not ok(k=(9, 2)) and not ok(k=(2, 9))
    assert not ok(stride=(5, 2)) and not ok(stride=(2, 5)) and not ok(pad=(2, 0)) and not ok(pad=(0, 2)) and not ok(op=(2, 0)) and not ok(op=(0, 2))
    assert not ok(rs=0) and not ok(rs=17) and not ok(rs=-1) and not ok(C=0) and not ok(K=0) and not ok(k=(0, 2)) and not ok(stride=(0, 2))
    assert not ok(pad=(-1, 0)) and not ok(op=(0, -1))
    # the accumulator bound: ceil(R / sh) ceil(S / sw) C 2^14 + 2^16 + (255 << rs) < 2^31 - 1
    assert ok(C=2031, k=(8, 8), stride=(1, 1), rs=16) and not ok(C=2032, k=(8, 8), stride=(1, 1), rs=16)
    assert ok(C=8124, k=(8, 8), stride=(2, 2), rs=16) and not ok(C=8128, k=(8, 8), stride=(2, 2), rs=16)
    assert ok(C=131000, k=(2, 2), rs=1) and not ok(C=131072, k=(2, 2), rs=1)
    L = _native.lib()
    assert L.fq_deconv2d_i8_packed_bytes(5, 3, 3, 3) == 16 * 9 * 16 and L.fq_deconv2d_i8_packed_bytes(17, 33, 4, 2) == 48 * 8 * 32
    assert L.fq_deconv2d_i8_packed_bytes(0, 3, 3, 3) == 0


@no_gpu
def test_every_refusal_by_return_code_and_nothing_is_written():
    from common.quantity import _native
    L = _native.lib()
    raw = ctypes.create_string_buffer(b"\x55" * (8192 + 64), 8192 + 64)
    base = (ctypes.addressof(raw) + 63) & ~63
    px, pw, pb, py = (ctypes.c_void_p(base + off) for off in (0, 2048, 4096, 6144))
    #       x   w   qb  q  Cpad Kpad relu N  H  W  C  K  R  S sh sw ph pw oh ow rs ob
    good = (px, pw, pb, py, 16, 16, 0, 1, 2, 2, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0)

    def put(i, v, base=good):
        return base[:i] + (v,) + base[i + 1:]

    invalid = {
        "null x": put(0, None), "null w": put(1, None), "null qbias": put(2, None), "null q": put(3, None),
        "misaligned x": put(0, ctypes.c_void_p(px.value + 4)), "misaligned w": put(1, ctypes.c_void_p(pw.value + 8)),
        "misaligned q": put(3, ctypes.c_void_p(py.value + 4)), "misaligned qbias": put(2, ctypes.c_void_p(pb.value + 2)),
        "Cpad": put(4, 32), "Kpad": put(5, 32), "N < 0": put(7, -1), "H < 1": put(8, 0), "W < 1": put(9, 0), "C < 1": put(10, 0),
        "K < 1": put(11, 0), "R < 1": put(12, 0), "S < 1": put(13, 0), "stride 0": put(14, 0), "pad < 0": put(16, -1),
        "outpad < 0": put(19, -1), "rs 121": put(20, 121), "ob 121": put(21, 121), "ob -121": put(21, -121),
        "no output plane": (px, pw, pb, py, 16, 16, 0, 1, 1, 1, 8, 8, 3, 3, 1, 1, 2, 2, 0, 0, 7, 0),
    }
    f = L.fq_deconv2d_i8_resident
    for what, a in invalid.items():
        assert f(*a, None) == INVALID, what
    unsupported = {
        "kernel 9": put(12, 9), "S = 9": put(13, 9), "stride 5": put(15, 5), "pad == kernel": put(16, 2), "outpad == stride": put(18, 2),
        "rs 0": put(20, 0), "rs 17": put(20, 17), "rs -3": put(20, -3),
        "an input of 2^31 bytes": put(7, 1 << 25, put(8, 2, put(9, 2))), "N H W past 2^31": put(8, 1 << 20, put(9, 1 << 20)),
        "an output of 2^30 bytes": put(7, 1 << 22, put(8, 2, put(9, 2))),
        "an accumulator past int32": (px, pw, pb, py, 8128, 16, 0, 1, 1, 1, 8128, 8, 8, 8, 2, 2, 0, 0, 0, 0, 16, 0),
        "a wrong scalar beats a null pointer": (None, None, None, None) + put(12, 9)[4:],
    }
    for what, a in unsupported.items():
        assert f(*a, None) == UNSUPPORTED, what
    assert f(*((None, None, None, None) + put(7, 0)[4:]), None) == 0                         # N == 0: FQ_OK without a launch
    assert f(*((None, None, None, None) + put(7, 0, put(12, 9))[4:]), None) == UNSUPPORTED   # ... but a wrong scalar is still refused
    g = L.fq_deconv2d_i8_resident_act
    act = good[:6] + (-5, 100) + good[7:]
    for lo, hi in ((1, 100), (-129, 100), (-5, 128), (-5, -1)):
        assert g(*(act[:6] + (lo, hi) + act[8:]), None) == INVALID
    assert g(*((None, None, None, None) + act[4:13] + (9,) + act[14:]), None) == UNSUPPORTED
    assert g(*((None, None, None, None) + act[4:8] + (0,) + act[9:]), None) == 0
    assert raw.raw == b"\x55" * (8192 + 64)


# ---------------------------------------------------------------- 4. the kernel's guards and address arithmetic on the host
def test_the_walker_builds_with_the_sanitizers_and_passes(tmp_path):
    """csrc/fq_deconv_i8_geom.h compiled as host code with the address and undefined-behaviour sanitizers:
    scripts/deconv_geom_check.cpp checks the `_supported` table and the guard's order, then walks every lane of every launch --
    every load inside x or the pack and aligned, every output byte written exactly once, every tap the rule's, the digit walk
    against the division -- over the GPU tests' cases and the model's launch shapes."""
    exe = str(tmp_path / "deconv_geom_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pytorch-quantity_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "scripts", "deconv_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("deconv_geom_check: OK") and not out.stderr, out.stdout + out.stderr
    cases = dn.kernel_cases() + [dn.BIG_CASE] + dn.model_launches()
    args = ["%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (c["N"], c["H"], c["W"], c["C"], c["K"], c["kernel"][0], c["kernel"][1], c["stride"][0],
                                                        c["stride"][1], c["pad"][0], c["pad"][1], c["outpad"][0], c["outpad"][1]) for c in cases]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("deconv_geom_check: OK") and len(lines) == len(cases) + 1 and not out.stderr, out.stdout + out.stderr
    rows = [re.match(r"case (\S+): items (\d+) blocks (\d+) KW (\d+)$", ln) for ln in lines[:-1]]
    assert all(rows)
    for c, row in zip(cases, rows):
        assert int(row.group(2)) == dn.items(c) and int(row.group(3)) == min(dn.items(c), dn.MAX_BLOCKS), c
    assert int(rows[len(dn.kernel_cases())].group(2)) > dn.MAX_BLOCKS
    header = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_deconv_i8_geom.h")).read()
    assert re.search(r"kDcTilePix = %d;" % dn.BLOCK_PIX, header) and re.search(r"kDcMaxBlocks = %d;" % dn.MAX_BLOCKS, header)


# ---------------------------------------------------------------- 5. NewConvTranspose2d
def test_the_layer_alone_default_form_and_own_kernel_give_the_same_tensor():
    from common.quantity import resident
    x = torch.randn(3, 16, 5, 4, generator=torch.Generator().manual_seed(3))
    with dd.installed():
        for k, s, p, op in dn.KSPO:
            m = dn.deconv(16, 8, k, 4, 3, stride=s, padding=p, output_padding=op).eval()
            assert isinstance(m.Conv, nn.ConvTranspose2d) and m.rs_bit == m.weight_bit + 1
            with torch.no_grad():
                want = m(x)
            assert not dd.calls and "_w_dc" not in m.__dict__ and m._deconv_left(m.Conv) is None and not m._deconv_ok(m.Conv)
            m.use_deconv_i8 = True
            with torch.no_grad():
                got = m(x)
            assert len(dd.calls) == 1 and torch.equal(got, want) and float(want.abs().max()) > 0 and got.dtype == torch.float32
            del dd.calls[:]
            assert "_w_dc" in m.__dict__ and "_w_dc" not in pickle.loads(pickle.dumps(m)).__dict__
            assert resident.resident_of(got) is None


def test_per_channel_weight_bits_raise_naming_the_layer():
    from common.quantity import NewConvTranspose2d
    info = {"weight_bit": [6] * 8, "bias_bit": 4, "input_bit": 4, "output_bit": 4}
    with pytest.raises(ValueError, match="decoder.up1"):
        NewConvTranspose2d(nn.ConvTranspose2d(16, 8, 2, stride=2), info, name="decoder.up1")
    with pytest.raises(ValueError, match="per-channel"):
        NewConvTranspose2d(nn.ConvTranspose2d(16, 8, 2, stride=2), info)


# ---------------------------------------------------------------- 6. what is planned
@pytest.mark.parametrize("variant", dn.TOY_VARIANTS)
def test_a_toy_net_is_planned_and_keeps_its_outputs(variant):
    from common.quantity import resident
    x = dn.example()
    with dd.installed():
        net = dn.ToyNet(variant).eval()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, **net.kw)
        off_plans = resident.describe(net)
        with torch.no_grad():
            off_out = net(x)
        assert not dd.calls and "up" not in off_plans and not off_plans.deconv_left and "resident_deconvs" not in off
        for name in net.fronts:
            assert off_plans[name].emit_f32, name                              # the layer reads fp32: its source leaves as fp32
        on = resident.enable(net, x, deconv=True, **net.kw)
        plans = resident.describe(net)
        assert set(on) == set(off) | {"resident_deconvs"} and on["resident_deconvs"] == 1 and not plans.deconv_left
        assert on["resident_convs"] == off["resident_convs"] + 1
        assert on["fp32_outputs"] < off["fp32_outputs"] or variant == "dc_out"
        for name in net.fronts:
            assert plans[name].emit_int and not plans[name].emit_f32, (name, plans[name])
        p = plans["up"]
        assert (p.emit_f32, p.emit_int) == ((True, False) if variant == "dc_out" else (False, True)), p
        assert not p.defer and not p.depthwise and not p.grouped and p.narrow_bit == net.up.output_bit
        assert (p.relu, p.clip) == {"dc_relu": (True, False), "dc_relu6": (True, True)}.get(variant, (False, False))
        if p.relu:
            assert isinstance(net.ru.__dict__.get("forward"), resident._ReluPassThrough)
        if variant == "act_dc":
            assert on["resident_activations"] == 1 and off["resident_activations"] == 0 and plans["act"].narrow_bit == 3
        if variant == "dc_cat_rq":
            assert on["requant_concats"] == 1 and off["requant_concats"] == 0
        if variant == "dc_cat":
            assert on["resident_concats"] == 1 and off["resident_concats"] == 0
        if variant == "dc_add":
            assert on["resident_adds"] == 1 and off["resident_adds"] == 0 and on["fused_conv_adds"] <= 1 and not plans["up"].defer
        del dd.calls[:]
        with torch.no_grad():
            got = net(x)
            assert torch.equal(got, plain) and torch.equal(got, off_out) and float(plain.abs().max()) > 0
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        assert len(dd.calls) == 3 and all(c[6:8] == (p.relu, (0, 96) if p.clip else None) for c in dd.calls), dd.calls
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert "_w_dc" in net.up.__dict__ and "_w_dc" not in again.up.__dict__
        assert "up" in resident.describe(again)
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and not resident.describe(net).deconv_left and "_resident" not in net.up.__dict__
        del dd.calls[:]
        with torch.no_grad():
            assert torch.equal(net(x), plain)
        assert not dd.calls


# ---------------------------------------------------------------- 7. what stays an fp32 producer, and why
@pytest.mark.parametrize("variant", sorted(dn.DECLINED))
def test_a_declined_layer_stays_fp32_and_describe_says_why(variant):
    from common.quantity import resident
    with dd.installed():
        net = dn.DeclinedNet(variant).eval()
        x = dn.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x)
        off_rows = _rows(resident.describe(net))
        on = resident.enable(net, x, deconv=True)
        plans = resident.describe(net)
        assert on["resident_deconvs"] == 0 and "up" not in plans
        assert list(plans.deconv_left) == ["up"] and dn.DECLINED[variant] in plans.deconv_left["up"], plans.deconv_left
        assert _rows(plans) == off_rows and {k: v for k, v in on.items() if k != "resident_deconvs"} == off       # the off arm's plan
        if variant == "shift":
            assert net.up.rs_bit == 17
        with torch.no_grad():
            assert torch.equal(net(x), plain)
        assert not dd.calls


def test_the_ok_net_of_the_declined_family_is_planned():
    from common.quantity import resident
    with dd.installed():
        net = dn.DeclinedNet("ok").eval()
        on = resident.enable(net, dn.example(), deconv=True)
        assert on["resident_deconvs"] == 1 and not resident.describe(net).deconv_left


# ---------------------------------------------------------------- 8. golden G28
def test_g28_both_up_convolutions_are_nodes_with_one_input(g28):
    ref, _arrays = g28
    info = ref["net_info"]
    ups = [k for k in ref["net_info_order"] if info[k]["type"] == "ConvTranspose2d"]
    assert len(ups) == 2 and all(len(info[k]["inputs"]) == 1 for k in ups)
    q = ref["quantity_information"]
    assert q["up1"]["layer_type"] == q["up2"]["layer_type"] == "ConvTranspose2d" and ref["seed"] == dn.G28_SEED
    assert ref["twin"]["quantity_information"]["up1"]["layer_type"] == "Conv2d"
    for key in ("input_bit", "output_bit", "weight_bit", "bias_bit"):
        assert ref["twin"]["quantity_information"]["up1"][key] == ref["twin"]["head_quantity_information"]["up1"][key]


def _calibrated(make, shape, oracle):
    """One float model through the product's CPU engine on the SHIPPED settings: (what discovery and the tables gave, the
    Reconstruction over a fresh copy, its quantity information, the work directory) -- inside product_workdir."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    q = CpuQuantity(make())
    got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
           "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
    q.activation_quantize(an.integer_batches(3, shape, dn.G28_CALIB_SEED))
    wd = os.path.join(os.getcwd(), "workdir")
    got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
    q.weight_quantize()
    got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
    q.rewrite_weight()
    got["weight_table_rewritten"] = open(os.path.join(wd, "weight.table")).read()
    rec = Reconstruction(make())
    info = rec.get_quantity_information()
    got["recon_layers"] = sorted(info.keys())
    got["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()}
    return got, rec, info, wd


def test_g28_discovery_and_tables_match_the_reference_byte_for_byte(g28, oracle):
    """The reference's graph discovery, merge groups, feat.table, both weight.tables and quantity information of the G28 net through
    the oracle-backed CPU engine on the SHIPPED settings.  On the parent discovery stops at the layer behind the first
    up-convolution ("Can't find the input tensor of ...")."""
    ref, _arrays = g28
    shape = dn.G28_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2):
        got, _rec, _info, _wd = _calibrated(dn.g28_net, shape, oracle)
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table",
                    "weight_table_rewritten", "recon_layers", "quantity_information"):
            assert got[key] == ref[key], key


def test_g28_twin_logits_from_newconvtranspose2d_with_the_switch_off_on_and_all_fourteen(g28, oracle):
    """The net that ends behind conv2, calibrated by the product's CPU engine: the tables the reference wrote for it AND for its
    twin (they are the same bytes), and the logits of the reference's own ReconModel of the twin, bit for bit, from ReconModel's
    NewConvTranspose2d: plain, per-instance own kernel, and under resident.enable with the switch off, on, and all fourteen."""
    from common.quantity import NewConvTranspose2d, resident
    ref, arrays = g28
    shape = dn.G28_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2):
        got, rec, info, wd = _calibrated(lambda: dn.g28_net(head_only=True), shape, oracle)
        for key in ("feat_table", "weight_table", "weight_table_rewritten"):
            assert got[key] == ref["twin"][key], key
        assert got["quantity_information"] == ref["twin"]["head_quantity_information"]
        for key in ("net_info", "net_info_order", "merge_groups", "cared_op_layer_names", "layers_num"):
            assert got[key] == ref["twin"]["head_" + key], key
        x = an.integer_input(shape, dn.G28_INPUT_SEED)
        np.testing.assert_array_equal(x.numpy(), arrays["x"])
        with torch.no_grad():
            np.testing.assert_array_equal(dn.g28_net(head_only=True)(x).numpy(), arrays["twin_float"])
            np.testing.assert_array_equal(dn.g28_twin()(x).numpy(), arrays["twin_float"])
        want = arrays["logits_twin_recon"]
        with dd.installed_all():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            assert isinstance(net.up1, NewConvTranspose2d) and isinstance(net.up1.Conv, nn.ConvTranspose2d)
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), want)
                assert not dd.calls
                net.up1.use_deconv_i8 = True
                np.testing.assert_array_equal(net(x).numpy(), want)
                assert len(dd.calls) == 1
                net.up1.use_deconv_i8 = False
                for kw in ({}, {"deconv": True}, ALL14):
                    summary = resident.enable(net, x, **kw)
                    np.testing.assert_array_equal(net(x).numpy(), want, err_msg=str(kw))
                    np.testing.assert_array_equal(net(x[:1]).numpy(), want[:1], err_msg=str(kw))
                    plans = resident.describe(net)
                    if kw:
                        assert summary["resident_deconvs"] == 1 and not plans.deconv_left and plans["up1"].relu
                        assert not plans["conv1"].emit_f32 and not plans["up1"].emit_f32 and summary["fp32_outputs"] == 1
                    else:
                        assert "up1" not in plans and plans["conv1"].emit_f32 and summary["fp32_outputs"] == 2


def test_g28_full_net_logits_are_the_exact_integer_rule(g28, oracle):
    """The whole G28 net as ReconModel builds it, held against include/fq.h's rule written out in numpy layer by layer (Quantity ->
    exact integer sums -> round-half-away shift, saturate, bias, Sp -> DeQuantity), plain and planned; ReconTest leaves both
    up-convolutions float."""
    from common.quantity import NewConvTranspose2d, resident
    from tools import Reconstruction
    ref, arrays = g28
    shape = dn.G28_SHAPE
    q = copy.deepcopy(ref["quantity_information"])
    x = an.integer_input(shape, dn.G28_INPUT_SEED)

    def quantity(t, bit):
        return np.clip(np.rint(t.astype(np.float64) * 2.0 ** bit), -128, 127).astype(np.int64)

    def layer(t, name, mod, relu):
        i = q[name]
        xi = quantity(t, i["input_bit"])                                                       # [N, C, H, W]
        w = np.clip(np.rint(mod.weight.detach().numpy().astype(np.float64) * 2.0 ** i["weight_bit"]), -128, 127).astype(np.int64)
        b = np.clip(np.rint(mod.bias.detach().numpy().astype(np.float64) * 2.0 ** i["bias_bit"]), -128, 127)
        N, C, H, W = xi.shape
        c = dn.case(N, H, W, C, w.shape[1] if isinstance(mod, nn.ConvTranspose2d) else w.shape[0], mod.kernel_size, mod.stride, mod.padding,
                    getattr(mod, "output_padding", (0, 0)), rs=i["weight_bit"] + i["input_bit"] - i["output_bit"], relu=relu)
        xn = np.zeros((N, H, W, dn.pad16(C)), dtype=np.int8)
        xn[..., :C] = np.moveaxis(xi, 1, -1)
        if isinstance(mod, nn.ConvTranspose2d):
            acc = dn.rule_acc(xn, w, c)
        else:
            from oracle import fq_oracle
            acc = np.moveaxis(fq_oracle.conv2d_int(xi, w, mod.stride, mod.padding), 1, -1)
        out = dn.int_tail(acc, b.astype(np.float32), c)[..., :c["K"]].astype(np.float64) * 2.0 ** -i["output_bit"]
        return np.moveaxis(out, -1, 1)

    f = dn.g28_net()
    t = layer(x.numpy(), "conv1", f.conv1, 1)
    t = layer(t, "up1", f.up1, 1)
    t = layer(t, "conv2", f.conv2, 0)
    t = layer(t, "up2", f.up2, 0)
    want = layer(t, "conv3", f.conv3, 0).astype(np.float32)
    assert want.shape == (4, 3, 64, 64) and want.std() > 0
    with dd.installed_all():
        net = dn.rebuild(dn.g28_net(), q)
        assert isinstance(net.up1, NewConvTranspose2d) and isinstance(net.up2, NewConvTranspose2d)
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).numpy(), want)
            for kw in ({}, {"deconv": True}, ALL14):
                summary = resident.enable(net, x, **kw)
                np.testing.assert_array_equal(net(x).numpy(), want, err_msg=str(kw))
                if kw:
                    # (conv3 has 4 input channels: a stem-like layer, which folds its width into the channels and reads fp32 -- so
                    #  up2 writes fp32 for it, and conv3 is the model output)
                    assert summary["resident_deconvs"] == 2 and summary["fp32_outputs"] == 2 and summary["int_only_outputs"] == 3
                    plans = resident.describe(net)
                    assert not plans["conv1"].emit_f32 and not plans["up1"].emit_f32 and not plans["conv2"].emit_f32 and plans["up2"].emit_f32
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2):
        info = {k: dict(v, layer=None) for k, v in q.items()}
        test_model = Reconstruction(dn.g28_net()).ReconTest(info, os.path.join(os.getcwd(), "workdir_recontest.pth"))
        assert type(test_model.up1) is nn.ConvTranspose2d and type(test_model.up2) is nn.ConvTranspose2d
        assert type(test_model.conv1).__name__ == "TestConv"


# ---------------------------------------------------------------- 9. the random family
def test_twenty_random_nets_keep_their_outputs_under_the_switch_alone_and_under_all_fourteen():
    """Whatever the plan takes or leaves, the outputs are the fp32-boundary model's, at the planned batch size and at one.  At least
    80 % of the drawn up-convolutions are planned: the generator draws a declined form (groups 2, dilation 2, a shift of 17 or
    more) for about one stage in seven; 49 are drawn and 42 planned on the CPU doubles (the counts are printed)."""
    from common.quantity import resident
    drawn = planned = 0
    with dd.installed_all():
        for seed in dn.SEEDS:
            m = dn.RandomDeconvNet(seed).eval()
            x = m.example()
            with torch.no_grad():
                plain = m(x)
            for kw in ({"deconv": True}, ALL14):
                on = resident.enable(m, x, **kw)
                with torch.no_grad():
                    assert torch.equal(m(x), plain) and torch.equal(m(x[:1]), plain[:1]), (seed, kw)
                plans = resident.describe(m)
                left = plans.deconv_left
                assert on["resident_deconvs"] + len(left) == len(m.ups), (seed, on, left)
                for name, expected in m.ups:
                    assert (name in plans) == expected and (name in left) != expected, (seed, name, left)
            drawn += len(m.ups)
            planned += sum(name in plans for name, _e in m.ups)
            resident.disable(m)
    print("random deconv nets: %d up-convolutions drawn, %d planned" % (drawn, planned))
    assert planned >= 0.8 * drawn
