"""What keeping the channel split and the channel shuffle in int8 is worth inside a network: ShuffleNetV2 1.0x
(model/shufflenetv2/ShuffleNetV2_fabu.py) at 256 images of 224 x 224, the resident int8-sim forward under
resident.enable(net, x, depthwise=True, concat=True) against (..., depthwise=True, concat=True, shuffle=True), the two arms
alternating in one process, timed with device events around `iters` forwards.

    python scripts/shuffle_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model gets seeded BatchNorm statistics (as bench.py gives ResNet-50), is folded (merge_bn) and calibrated on the GPU on two
batches of 32 seeded images; Reconstruction builds one ReconModel per arm.  Each arm's logits are checked against its plain
forward and its plan summary and kernel launch counts are printed; with both arms the logits of the two arms must be identical
(asserted).  `rounds` (at least five) timings of each arm; every round, the median and the spread of each arm and the median
on / off ratio are printed.  The `on` arm also reports what describe() says was left to torch, the bytes its fq_shuffle_i8_nhwc
launches move per forward -- the sum over the launches of N H W (Cpad_in + Cpad_out) -- and the bytes per second the kernel
reaches on those launches alone (each distinct launch timed on its own, `iters` times between two device events), next to the
8 TB/s of the README as a ratio.

`--arms off` never names the new switch: this file and model/shufflenetv2/ copied into a checkout of the commit before them, with
the Slice marker and the two names of tools/configs.yml added, give the baseline.
"""
import argparse
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


def build_model(hw, device):
    from common.quantity import merge_bn
    from model.shufflenetv2.ShuffleNetV2_fabu import ShuffleNetV2
    torch.manual_seed(0)
    model = ShuffleNetV2(num_classes=1000, width_mult=1.0, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def launch_bytes(launches):
    """sum over (N, H, W, Cpad_in, c_in, c_off, c, groups) of N H W (Cpad_in + pad16(c)): one read of the row, one write"""
    return sum(n * h * w * (cpad_in + (c + 15) // 16 * 16) for (n, h, w, cpad_in, _c_in, _c_off, c, _g) in launches)


def recorded_launches(net, x):
    """[(N, H, W, Cpad_in, c_in, c_off, c, groups), ...] of the fq_shuffle_i8_nhwc launches of one forward"""
    from common.quantity import _native
    seen = []
    real = _native.shuffle_i8_nhwc

    def spy(x_q, c_in, c_off, c, groups, out=None):
        seen.append(tuple(int(v) for v in x_q.shape) + (int(c_in), int(c_off), int(c), int(groups)))
        return real(x_q, c_in, c_off, c, groups, out)

    _native.shuffle_i8_nhwc = spy
    try:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    finally:
        _native.shuffle_i8_nhwc = real
    return seen


def kernel_rate(launches, iters, say):
    from common.quantity import _native
    total_bytes, total_ms = 0, 0.0
    for key in sorted(set(launches)):
        n, h, w, cpad_in, c_in, c_off, c, g = key
        xq = torch.randint(-128, 128, (n, h, w, cpad_in), dtype=torch.int8, device="cuda")
        out = torch.empty(n, h, w, (c + 15) // 16 * 16, dtype=torch.int8, device="cuda")
        _native.shuffle_i8_nhwc(xq, c_in, c_off, c, g, out=out)                       # warm
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            _native.shuffle_i8_nhwc(xq, c_in, c_off, c, g, out=out)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / iters
        b = launch_bytes([key])
        count = launches.count(key)
        say("  kernel %dx%dx%d Cpad_in %d c_off %d C %d groups %d: %d per forward, %.1f MB, %.4f ms, %.3f TB/s"
            % (n, h, w, cpad_in, c_off, c, g, count, b / 1e6, ms, b / ms / 1e9))
        total_bytes += b * count
        total_ms += ms * count
    rate = total_bytes / total_ms * 1e3
    say("on: fq_shuffle_i8_nhwc alone, all launches of one forward: %.1f MB in %.3f ms = %.3f TB/s, %.3f of %.0f TB/s"
        % (total_bytes / 1e6, total_ms, rate / 1e12, rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))


def run(a, arms, say):
    from common.quantity import _native, resident
    from tools import Quantity, Reconstruction
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(32, 3, 224, 224, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(224, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(224, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s.pth" % key)
    say("resident: ShuffleNetV2 1.0x, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        if key == "on":
            plan = resident.enable(net, x, depthwise=True, concat=True, shuffle=True)
        else:
            plan = resident.enable(net, x, depthwise=True, concat=True)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident logits differ from the plain forward (%s)" % key
        logits[key] = out
        _native.conv_variant_log = {}
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: integer-kernel launches per forward %s" % (key, dict(sorted(_native.conv_variant_log.items()))))
        _native.conv_variant_log = None
        if key == "on":
            left = resident.describe(net).shuffle_left
            say("on: shuffles and slices left to torch: %s" % (dict(left) if left else "none"))
            launches = recorded_launches(net, x)
            say("on: %d fq_shuffle_i8_nhwc launches per forward move %.1f MB (sum of N H W (Cpad_in + Cpad_out))"
                % (len(launches), launch_bytes(launches) / 1e6))
            if launches:
                kernel_rate(launches, a.iters, say)
    if len(arms) == 2:
        assert torch.equal(logits["off"], logits["on"]), "the two arms disagree"
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

    say("command: python scripts/shuffle_cost.py " + " ".join(sys.argv[1:]))
    tmp = bench.make_workdir(1, "1,3,224,224", torch.cuda.current_device())       # cwd = its test/ directory
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
