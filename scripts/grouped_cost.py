"""What the grouped int8 kernel is worth inside a network: the resident int8-sim forward of the ResNeXt-50 32x4d-shaped model
(model/resnext/ResNeXt_fabu.py) at 224 x 224, resident.enable(net, x) against resident.enable(net, x, grouped=True), in one
process, alternating, timed with device events.

    python scripts/grouped_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model gets seeded BatchNorm statistics (as bench.py gives ResNet-50), is folded (merge_bn) and calibrated on the GPU on two
batches of 32 seeded images (activation_quantize, weight_quantize); Reconstruction builds one ReconModel per arm.  Each arm's
resident logits are checked against its plain forward (and the arms against each other), its plan summary and the kernel launch
counts of one forward (conv_variant_log) are printed, then every round times `iters` forwards of each arm; a line per round,
the spread of each arm and the median on / off ratio are printed.  The table of grouped layer shapes gives the algorithmic
bytes of each layer (int8 input + int8 output + weights) and its count of lane-dot4 instructions, which a kernel trace is read
against: run

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/grouped_cost.py --arms on  --rounds 1 --iters 3
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/grouped_cost.py --arms off --rounds 1 --iters 3

(runs of their own, no counters) for the per-kernel times.

`--arms off` calls resident.enable(net, x) without the new argument and touches nothing else that is new: this file and
model/resnext/ (plain torch modules) copied into a checkout of the commit before the grouped kernel give the baseline.
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


def build_model(hw, device):
    from common.quantity import merge_bn
    from model.resnext.ResNeXt_fabu import ResNeXt50
    torch.manual_seed(0)
    model = ResNeXt50(num_classes=1000, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
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
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s.pth" % key)
    return nets, tmp


def grouped_shapes(net, images):
    """(name, C, K, groups, kernel, stride, H, W, P, Q, shift, algorithmic bytes, lane-dot4 count) of every grouped layer that is
    not depthwise, from one hooked forward."""
    rows, hooks = [], []
    for name, m in net.named_modules():
        conv = getattr(m, "Conv", None)
        if isinstance(conv, torch.nn.Conv2d) and 1 < conv.groups < conv.in_channels:
            def hook(mod, inp, out, name=name, conv=conv):
                N, H, W, P, Q = inp[0].shape[0], inp[0].shape[2], inp[0].shape[3], out.shape[2], out.shape[3]
                cpad, kpad = (conv.in_channels + 15) // 16 * 16, (conv.out_channels + 15) // 16 * 16
                taps, cgi = conv.kernel_size[0] * conv.kernel_size[1], conv.in_channels // conv.groups
                nbytes = N * (H * W * cpad + P * Q * kpad) + kpad * taps * cgi
                dot4 = N * P * Q * conv.out_channels * taps * (cgi // 4)
                rows.append((name, conv.in_channels, conv.out_channels, conv.groups, conv.kernel_size[0], conv.stride[0], H, W, P,
                             Q, mod.rs_bit, nbytes, dot4))
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros(images, 3, 224, 224, device="cuda"))
    for h in hooks:
        h.remove()
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
    from common.quantity import _native, resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, tmp = build_nets(arms)
    say("model: ResNeXt-50 32x4d, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        if key == arms[0]:
            say("grouped layers (name, C -> K / groups, kernel, stride, HxW -> PxQ, shift, int8 in + int8 out + weights in MB and "
                "lane-dot4 in G for %d images; at 8 TB/s, at 6.3 TB/s, at 256 CUs x 128 lanes/clk x 2.4 GHz in us):" % a.images)
            for (name, C, K, G, k, st, H, W, P, Q, rs, nbytes, dot4) in grouped_shapes(net, a.images):
                say("  %-16s %4d -> %4d / %2d  %dx%d s%d  %3dx%-3d -> %3dx%-3d  rs %-3s %8.2f MB %6.3f G  %6.1f %6.1f %6.1f us"
                    % (name, C, K, G, k, k, st, H, W, P, Q, rs, nbytes / 1e6, dot4 / 1e9, nbytes / 8e6, nbytes / 6.3e6,
                       dot4 / (256 * 128 * 2.4e3)))
        plan = resident.enable(net, x, grouped=True) if key == "on" else resident.enable(net, x)
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
