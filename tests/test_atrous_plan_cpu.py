"""The atrous depthwise kernel's host side on a box without a GPU: fq_dwconv2d_dil_i8_supported at both sides of every limit,
NewConv2d._atrous_left's reasons, resident.enable(depthwise=True) with the layer attribute off and on (the kernel entry point is
an oracle-backed double on top of tests/depthwise_doubles.py), and the host walker over the GPU test's launches."""
import os
import subprocess

import numpy as np
import torch
from torch import nn

import atrous_cases
import depthwise_doubles
import depthwise_nets as dn
import native_doubles
from oracle import fq_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_supported_rule_at_both_sides_of_every_limit():
    from common.quantity import _native
    L = _native.lib()
    ok = dict(C=32, R=3, S=3, sh=1, sw=1, dh=2, dw=2, lo=7, hi=7)

    def ask(fn=L.fq_dwconv2d_dil_i8_supported, **kw):
        a = dict(ok, **kw)
        return fn(a["C"], a["R"], a["S"], a["sh"], a["sw"], a["dh"], a["dw"], a["lo"], a["hi"])

    taken = [{}, dict(C=1), dict(R=5, S=5), dict(dh=64, dw=64), dict(lo=1, hi=16), dict(dh=3, dw=3)]
    declined = [dict(C=0), dict(R=1, S=1), dict(R=7, S=7), dict(R=3, S=5), dict(dh=1, dw=1), dict(dh=65, dw=65), dict(dh=2, dw=3),
                dict(sh=2, sw=2), dict(sh=1, sw=2), dict(lo=0, hi=7), dict(lo=7, hi=17), dict(lo=8, hi=7)]
    assert [ask(**kw) for kw in taken] == [1] * len(taken)
    assert [ask(**kw) for kw in declined] == [0] * len(declined)
    assert ask(L.fq_dwconv2d_i8_supported) == 0 and ask(L.fq_dwconv2d_i8_supported, dh=1, dw=1) == 1    # the dense rule as it was
    assert _native.dwconv_dil_supported(32, 3, 3, (1, 1), (2, 2), 7) and not _native.dwconv_dil_supported(32, 3, 3, (1, 1), (1, 1), 7)
    assert _native.CONV_VARIANTS[17] == "depthwise_dilated" and L.fq_version() == 103


def _layer(conv, wb=5, ib=4, ob=4):
    from common.quantity import NewConv2d
    return NewConv2d(conv, {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob})


def test_atrous_left_names_a_reason_and_depthwise_ok_is_unchanged():
    from common.quantity import NewConv2d
    assert NewConv2d.use_atrous_i8 is False
    ok = _layer(nn.Conv2d(16, 16, 3, padding=2, dilation=2, groups=16))
    assert ok._atrous_left(ok.Conv) is None and not ok._atrous_ok(ok.Conv) and ok._atrous_ok(ok.Conv, True)
    ok.use_atrous_i8 = True
    assert ok._atrous_ok(ok.Conv) and not ok._depthwise_ok(ok.Conv, True)            # the dense rule still declines dilation
    for conv in (nn.Conv2d(8, 8, 5, padding=12, dilation=3, groups=8), nn.Conv2d(8, 8, 3, padding=0, dilation=64, groups=8)):
        assert _layer(conv)._atrous_left(conv) is None                                 # padding = the span, the largest dilation
    for word, conv, kw in [
            ("depthwise", nn.Conv2d(16, 16, 3, padding=2, dilation=2), {}),
            ("depthwise", nn.Conv2d(16, 32, 3, padding=2, dilation=2, groups=16), {}),
            ("padding", nn.Conv2d(16, 16, 3, padding="same", dilation=2, groups=16), {}),
            ("padding", nn.Conv2d(16, 16, 3, padding=2, dilation=2, groups=16, padding_mode="reflect"), {}),
            ("stride", nn.Conv2d(16, 16, 3, stride=2, padding=2, dilation=2, groups=16), {}),
            ("dilation", nn.Conv2d(16, 16, 3, padding=1, groups=16), {}),
            ("dilation", nn.Conv2d(16, 16, 3, padding=2, dilation=(2, 3), groups=16), {}),
            ("dilation", nn.Conv2d(16, 16, 3, padding=2, dilation=65, groups=16), {}),
            ("kernel size", nn.Conv2d(16, 16, 7, padding=6, dilation=2, groups=16), {}),
            ("span", nn.Conv2d(16, 16, 3, padding=(4, 5), dilation=2, groups=16), {}),
            ("shift", nn.Conv2d(16, 16, 3, padding=2, dilation=2, groups=16), {"wb": 0}),
            ("shift", nn.Conv2d(16, 16, 3, padding=2, dilation=2, groups=16), {"wb": [17] + [5] * 15})]:
        m = _layer(conv, **kw)
        why = m._atrous_left(m.Conv)
        assert why is not None and word in why and not m._atrous_ok(m.Conv, True), (word, why)
    dense = _layer(nn.Conv2d(16, 16, 3, padding=1, groups=16))
    assert dense._depthwise_ok(dense.Conv, True) and not dense._atrous_ok(dense.Conv, True)


def _dil_double(xq, wq, qbias, padding, dilation, rs, ob, relu):
    """dwconv2d_dil_i8_resident by the reference's chain, as depthwise_doubles.dwconv2d_i8_resident is for the dense kernel."""
    C = qbias.numel()
    x = np.ascontiguousarray(np.moveaxis(native_doubles._np(xq).astype(np.int32), -1, 1)[:, :C])
    w = np.ascontiguousarray(np.transpose(native_doubles._np(wq).astype(np.int32), (2, 0, 1))[:C, None])
    y = depthwise_doubles._tail(orc.conv2d_int(x, w, (1, 1), tuple(padding), tuple(dilation), groups=C), qbias,
                                depthwise_doubles._shifts(rs, C), ob)
    return native_doubles._to_i8_nhwc(np.maximum(y, np.float32(0)) if relu else y, ob, xq.shape[-1])


class _ToyNet(nn.Module):
    def __init__(self):
        super(_ToyNet, self).__init__()
        self.c1 = nn.Conv2d(3, 19, 3, padding=1)
        self.r1 = nn.ReLU(False)
        self.dw = nn.Conv2d(19, 19, 3, padding=2, dilation=2, groups=19)
        self.r2 = nn.ReLU6(False)
        self.c2 = nn.Conv2d(19, 8, 1)

    def forward(self, x):
        return self.c2(self.r2(self.dw(self.r1(self.c1(x)))))


def test_the_plan_takes_the_layer_only_with_the_attribute(monkeypatch):
    from common.quantity import resident
    with depthwise_doubles.installed() as nat:
        calls = []
        monkeypatch.setattr(nat, "dwconv2d_dil_i8_resident", lambda *a: (calls.append(a[4]), _dil_double(*a))[1])
        model = dn.seeded(_ToyNet().eval())
        net = dn.rebuild(model, dn.fixed_info(model))
        x = torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            plain = net(x)
        default = resident.enable(net, x)
        off = resident.enable(net, x, depthwise=True)
        plans = resident.describe(net)
        assert "dw" not in plans and plans["c1"].emit_f32 and off.get("resident_depthwise", 0) == 0      # an fp32 producer, as before
        assert off["fp32_outputs"] == default["fp32_outputs"]
        with torch.no_grad():
            assert torch.equal(net(x), plain) and not calls
        net.dw.use_atrous_i8 = True
        on = resident.enable(net, x, depthwise=True)
        plans = resident.describe(net)
        # planned: it reads c1's int8 (c1 writes no fp32 any more); without relu6=True the ReLU6 behind it stays a float module
        assert plans["dw"].depthwise and plans["dw"].emit_f32 and not plans["dw"].relu and not plans["c1"].emit_f32
        assert on["resident_depthwise"] == 1 and on["resident_convs"] == off["resident_convs"] + 1
        with torch.no_grad():
            assert torch.equal(net(x), plain)
        assert calls and all(tuple(d) == (2, 2) for d in calls)
        resident.disable(net)
        del calls[:]
        with torch.no_grad():
            assert torch.equal(net(x), plain)                       # no plan: the attribute alone runs the layer on the kernel
        assert len(calls) == 1


def test_the_walker_passes_over_the_gpu_tests_launches_under_the_sanitizers(tmp_path):
    """scripts/dwconv_dil_geom_check.cpp, a plain executable built with -fsanitize=address,undefined, walks every lane of every
    launch of tests/atrous_cases.py: no load outside the input, no store outside the output, every output dword written once."""
    exe = str(tmp_path / "dwconv_dil_geom_check")
    subprocess.check_call(["c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "dwconv_dil_geom_check.cpp")])
    out = subprocess.run([exe] + [atrous_cases.walker_arg(c) for c in atrous_cases.KERNEL_CASES], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
