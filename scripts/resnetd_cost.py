"""What the windowed average pool over a NewAdd sum is worth inside a network: the resident int8-sim forward of ResNet-50-D
(model/resnetd/ResNetD_fabu.py) at 224 x 224, resident.enable(net, x, avgpool=True) against
resident.enable(net, x, avgpool=True, sums=True), in one process, alternating, timed with device events.

    python scripts/resnetd_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model is seeded, its batch norms folded (merge_bn) and it is really calibrated on the GPU on two batches of 32 seeded images
(activation_quantize, weight_quantize); the convolution behind a shortcut pool gets the Eltwise's bit as its input bit.
Reconstruction builds one ReconModel per arm.  Each arm's resident logits are checked against its plain forward and against the
other arm's, its plan summary (with `fp32_outputs`) is printed, then every round times `iters` forwards of each arm; a line per
round, the median and spread of each arm and the median on / off ratio are printed.  The table of pools gives the algorithmic
bytes of each launch -- int16 source read, 2 N H W Cpad, plus int8 output written, N P Q Cpad -- and the kernel alone is timed at
those shapes with device events against the 8 TB/s of the HBM.  `--arms off` is the behaviour before the kernel existed: the
three sums in front of stages 2, 3 and 4 also leave as fp32, torch pools them and fq_quantize_i8_nhwc re-quantises the result.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/resnetd_cost.py --arms on --rounds 1 --iters 3

(a run of its own, no counters).
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

HBM_GBS = 8000.0


def build_model(hw, device):
    from common.quantity import merge_bn
    from model.resnetd.ResNetD_fabu import ResNet50D
    torch.manual_seed(0)
    model = ResNet50D(num_classes=1000, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in model.named_parameters():            # He-style spread for the weights; the batch norms keep gamma 1
            if p.dim() > 1:
                scale = (2.0 / max(1, p[0].numel())) ** 0.5
                if name.endswith("conv3.weight") and "layer" in name:
                    scale *= 0.25                            # a bottleneck's last layer: keeps sixteen residual adds from blowing up
                p.copy_(torch.randn(p.shape, generator=g) * scale)
            elif name.endswith("bias"):                     # (a folded bias of exactly zero has no weight bit: the quantiser takes log2 of it)
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return merge_bn(model.eval()).to(device)


def build_nets(arms):
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,224,224", torch.cuda.current_device())          # cwd = its test/ directory
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(32, 3, 224, 224, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(224, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(224, "cuda"))
        info = rec.get_quantity_information()
        nets[key] = rec.ReconModel(info, "./workdir/recon_%s.pth" % key)
    return nets, info, tmp


def pool_shapes(net, images):
    """(name, channels, kernel, stride, padding, H, W, P, Q, algorithmic bytes) of every windowed nn.AvgPool2d, from one hooked
    forward (the whole-plane pool in front of the head is served by fq_avgpool_global_nhwc and is left out)."""
    rows, hooks = [], []
    pad = lambda c: (c + 15) // 16 * 16
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.AvgPool2d):
            def hook(mod, inp, out, name=name):
                n, c, H, W = inp[0].shape
                P, Q = out.shape[2:]
                if (P, Q) != (1, 1):
                    rows.append((name, c, mod.kernel_size, mod.stride, mod.padding, H, W, P, Q, n * pad(c) * (2 * H * W + P * Q)))
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros(images, 3, 224, 224, device="cuda"))
    for h in hooks:
        h.remove()
    return rows


def time_kernel(shapes, images, iters=200):
    """The kernel alone at the model's pool shapes (count_include_pad, shift 0, no ReLU), device events around `iters` launches on
    random int16 data: (name, microseconds per launch, algorithmic GB/s)."""
    from common.quantity import _native
    pair = lambda v: (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))
    rows = []
    for (name, c, k, s, p, H, W, _P, _Q, nbytes) in shapes:
        q = torch.randint(-32768, 32768, (images, H, W, (c + 15) // 16 * 16), dtype=torch.int16, device="cuda")
        out = _native.avgpool_i16_nhwc(q, c, pair(k), pair(s), pair(p), True, 0, False)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            _native.avgpool_i16_nhwc(q, c, pair(k), pair(s), pair(p), True, 0, False, out=out)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) / iters * 1e3
        rows.append((name, us, nbytes / us / 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from common.quantity import resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, info, tmp = build_nets(arms)
    say("model: ResNet-50-D, really calibrated, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0, "the logits are constant"
        if key == arms[0]:
            shapes = pool_shapes(net, a.images)
        plan = resident.enable(net, x, avgpool=True, sums=True) if key == "on" else resident.enable(net, x, avgpool=True)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident logits differ from the plain forward (%s)" % key
        logits[key] = (out, plain)
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d" % (key, plan["fp32_outputs"]))
        if key == arms[-1]:
            taken = resident.describe(net)
            for name, why in sorted(taken.avgpool_left.items()):
                say("  left to torch: %s: %s" % (name, why))
            say("windowed pools (name, channels, kernel / stride / padding, plane -> plane, int16 source read + int8 output written"
                " in MB for %d images, planned by this arm):" % a.images)
            total = 0
            for (name, c, k, s, p, H, W, P, Q, nbytes) in shapes:
                on = name in taken
                say("  %-24s %4d  %s / %s / %s  %3dx%-3d -> %3dx%-3d %8.2f MB  %s" % (name, c, k, s, p, H, W, P, Q, nbytes / 1e6,
                                                                                   "resident" if on else "fp32 form"))
                total += nbytes if on else 0
            say("  all resident pools of one forward: %.2f MB" % (total / 1e6))
            say("fq_avgpool_i16_nhwc alone at these shapes (back-to-back launches, device events; algorithmic bytes / time, and that "
                "as a share of %.0f TB/s):" % (HBM_GBS / 1e3))
            for (name, us, gbs) in time_kernel(shapes, a.images):
                say("  %-24s %8.1f us  %7.0f GB/s  %5.1f %%" % (name, us, gbs, 100.0 * gbs / HBM_GBS))
    if len(arms) == 2:
        assert torch.equal(logits["off"][0], logits["on"][0]) and torch.equal(logits["off"][1], logits["on"][1]), "the two arms disagree"
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
        say("%s: median %.3f ms, min %.3f, max %.3f, spread (max - min) / median %.3f, %.0f images/s"
            % (key, float(np.median(v)), min(v), max(v), (max(v) - min(v)) / float(np.median(v)), a.images / float(np.median(v)) * 1e3))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
