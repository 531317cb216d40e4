"""What keeping an elementwise activation that is no clamp in int8 is worth inside a network: YoloTiny
(model/yolotiny/YoloTiny_fabu.py, every convolution followed by nn.LeakyReLU(0.1)) at 256 images of 416 x 416 or 224 x 224, the
resident int8-sim forward under resident.enable(net, x, depthwise=False, concat=True, shuffle=True) against
(..., activations=True), the two arms alternating in one process, timed with device events around `iters` forwards.

    python scripts/activation_cost.py [--arms both|off|on] [--hw 416] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model gets seeded BatchNorm statistics (as bench.py gives ResNet-50), is folded (merge_bn) and calibrated on the GPU on two
batches of 16 seeded images; Reconstruction builds one ReconModel per arm.  Each arm's logits are checked against its plain
forward and its plan summary is printed; with both arms the logits of the two arms must be identical (asserted).  `rounds` (at
least five) timings of each arm; every round, the median and the spread of each arm and the median on / off ratio are printed.
The `on` arm also reports what describe() says was left to torch, the number of fq_act_lut_i8_nhwc launches per forward and the
bytes they move -- the sum over the launches of 2 N H W Cpad, one read and one write --, and, launch by launch, the time of BOTH
forms of the lookup (csrc/fq_act_lut_i8.hip: form 0 the table in LDS, one byte read per element; form 1 the table in registers,
fetched with ds_bpermute_b32) against that bound at the 8 TB/s of the README.

`--arms off` never names the new switch.  Runs through scripts/ab_lib.py against another build of the library as well.
"""
import argparse
import ctypes
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12
OFF = dict(depthwise=False, concat=True, shuffle=True)


def build_model(device):
    from common.quantity import merge_bn
    from model.yolotiny.YoloTiny_fabu import YoloTiny
    torch.manual_seed(0)
    model = YoloTiny(num_outputs=255, width=32, heads=2)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def recorded_launches(net, x):
    """[(N, H, W, Cpad, C), ...] of the fq_act_lut_i8_nhwc launches of one forward"""
    from common.quantity import _native
    seen = []
    real = _native.act_lut_i8_nhwc

    def spy(x_q, c, table, out=None):
        seen.append(tuple(int(v) for v in x_q.shape) + (int(c),))
        return real(x_q, c, table, out)

    _native.act_lut_i8_nhwc = spy
    try:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    finally:
        _native.act_lut_i8_nhwc = real
    return seen


def kernel_rate(launches, iters, say):
    from common.quantity import _native
    fn = _native.lib().fq_debug_act_lut_i8_form
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    table = torch.randint(-128, 128, (256,), dtype=torch.int8, device="cuda")
    totals = {0: 0.0, 1: 0.0}
    total_bytes = 0
    for key in sorted(set(launches)):
        n, h, w, cpad, c = key
        xq = torch.randint(-128, 128, (n, h, w, cpad), dtype=torch.int8, device="cuda")
        out = torch.empty_like(xq)
        b = 2 * n * h * w * cpad
        count = launches.count(key)
        ms = {}
        for form in (0, 1, 0, 1):                                 # (each form twice, alternating; the later timing is kept)
            stream = _native._stream(xq)
            assert fn(xq.data_ptr(), out.data_ptr(), table.data_ptr(), n, h, w, c, cpad, form, stream) == 0      # warm
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn(xq.data_ptr(), out.data_ptr(), table.data_ptr(), n, h, w, c, cpad, form, stream)
            t1.record()
            torch.cuda.synchronize()
            ms[form] = t0.elapsed_time(t1) / iters
        say("  kernel %dx%dx%d C %d Cpad %d: %d per forward, %.1f MB, bound %.4f ms; LDS bytes %.4f ms (%.3f TB/s), bpermute %.4f ms (%.3f TB/s)"
            % (n, h, w, c, cpad, count, b / 1e6, b / HBM_BYTES_PER_S * 1e3, ms[0], b / ms[0] / 1e9, ms[1], b / ms[1] / 1e9))
        total_bytes += b * count
        for form in (0, 1):
            totals[form] += ms[form] * count
    for form, name in ((0, "LDS byte reads"), (1, "ds_bpermute_b32")):
        rate = total_bytes / totals[form] * 1e3
        say("on: fq_act_lut_i8_nhwc alone (%s), all launches of one forward: %.1f MB in %.3f ms = %.3f TB/s, %.3f of %.0f TB/s"
            % (name, total_bytes / 1e6, totals[form], rate / 1e12, rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))


def run(a, arms, say):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(16, 3, a.hw, a.hw, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model("cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model("cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s.pth" % key)
    say("resident: YoloTiny, %d images at %d x %d, arms %s" % (a.images, a.hw, a.hw, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.hw, a.hw)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, activations=True, **OFF) if key == "on" else resident.enable(net, x, **OFF)
        with torch.no_grad():
            out = net(x)
        assert all(torch.equal(o, p) for o, p in zip(out, plain)), "resident logits differ from the plain forward (%s)" % key
        logits[key] = out
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        if key == "on":
            left = resident.describe(net).activations_left
            say("on: activations left to torch: %s" % (dict(left) if left else "none"))
            launches = recorded_launches(net, x)
            say("on: %d fq_act_lut_i8_nhwc launches per forward move %.1f MB (sum of 2 N H W Cpad)"
                % (len(launches), sum(2 * n * h * w * cpad for (n, h, w, cpad, _c) in launches) / 1e6))
            if launches:
                kernel_rate(launches, a.iters, say)
        del plain
    if len(arms) == 2:
        assert all(torch.equal(f, n) for f, n in zip(logits["off"], logits["on"])), "the two arms disagree"
        say("logits: on == off == plain forward")
    per_arm = {key: [] for key in arms}
    for r in range(a.rounds):
        ms = {}
        for key in arms:
            net = nets[key]
            with torch.no_grad():
                net(x)                                            # warm
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    net(x)
                t1.record()
            torch.cuda.synchronize()
            ms[key] = t0.elapsed_time(t1) / a.iters
            per_arm[key].append(ms[key])
        say("round %d: " % r + ", ".join("%s %.3f ms" % (k, ms[k]) for k in arms) + " per %d-image forward" % a.images
            + (", ratio on / off %.3f" % (ms["on"] / ms["off"]) if len(arms) == 2 else ""))
    for key in arms:
        v = per_arm[key]
        med = float(np.median(v))
        say("%s: median %.3f ms, min %.3f, max %.3f, spread (max - min) / median %.3f, %.0f images/s"
            % (key, med, min(v), max(v), (max(v) - min(v)) / med, a.images / med * 1e3))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--hw", type=int, choices=[224, 416], default=416)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.rounds >= 5 or a.arms != "both", "at least five timings per arm"
    import bench
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python scripts/activation_cost.py " + " ".join(sys.argv[1:]))
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.hw, a.hw), torch.cuda.current_device())       # cwd = its test/ directory
    try:
        run(a, arms, say)
    finally:
        os.chdir(ROOT)
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
