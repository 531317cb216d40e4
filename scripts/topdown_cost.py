"""What the resident add with a nearest-upsampled operand is worth inside a network: the resident int8-sim forward of
ResNet-50-FPN (model/fpn/ResNetFPN_fabu.py) at 224 x 224, resident.enable(net, x, concat=True) against
resident.enable(net, x, concat=True, topdown=True), in one process, alternating, timed with device events.

    python scripts/topdown_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model is seeded, its batch norms folded (merge_bn) and it is really calibrated on the GPU on two batches of 32 seeded images
(activation_quantize, weight_quantize).  Reconstruction builds one ReconModel per arm.  Each arm's resident logits are checked
against its plain forward and against the other arm's, its plan summary (with `fp32_outputs`) is printed, then every round times
`iters` forwards of each arm; a line per round, the median and spread of each arm and the median on / off ratio are printed.
The two top-down steps are also timed one by one in each arm (device events around the step's lateral convolution, upsampling,
add and output convolution, summed): the first step has an int8 source and trades the fused conv + add of the `off` arm for a
convolution and an add-up launch, so it need not gain; the second reads the int16 sum and leaves fp32 in the `off` arm.  Last,
fq_add_up_resident alone is timed at the model's launch shapes against the bytes it moves -- lateral read, coarse operand read
once, outputs written -- and the 8 TB/s of the HBM.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/topdown_cost.py --arms on --rounds 1 --iters 3

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
STEPS = (("step 1 (int8 source)", ("lateral4", "up5", "Eltwise4", "output4")),
         ("step 2 (int16 sum source)", ("lateral3", "up4", "Eltwise3", "output3")))


def build_model(hw, device):
    from common.quantity import merge_bn
    from model.fpn.ResNetFPN_fabu import ResNet50FPN
    torch.manual_seed(0)
    model = ResNet50FPN(num_classes=1000, input_size=hw)
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


def add_shapes(net, images):
    """(name of the add, channels, factor, H, W of the output plane) of every add behind an upsampling, from one hooked forward."""
    rows, hooks, ups = [], [], {}
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.Upsample):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: ups.__setitem__(id(out), int(mod.scale_factor))))
        elif type(m).__name__ == "NewAdd":
            def hook(mod, inp, out, name=name):
                for t in inp:
                    if id(t) in ups:
                        rows.append((name, int(out.shape[1]), ups[id(t)], int(out.shape[2]), int(out.shape[3])))
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros(images, 3, 224, 224, device="cuda"))
    for h in hooks:
        h.remove()
    return rows


def time_kernel(shapes, images, iters=200):
    """fq_add_up_resident alone at the model's shapes, device events around `iters` launches on random data:
    (label, microseconds per launch, bytes moved, GB/s).  Step 1 as the plan runs it: int8 + int8 -> wide and narrow; step 2:
    int8 + int16 -> narrow."""
    from common.quantity import _native
    rows = []
    for i, (name, c, up, H, W) in enumerate(shapes):
        cpad = (c + 15) // 16 * 16
        first = i == 0
        x = torch.randint(-128, 128, (images, H, W, cpad), dtype=torch.int8, device="cuda")
        if first:
            y = torch.randint(-128, 128, (images, H // up, W // up, cpad), dtype=torch.int8, device="cuda")
        else:
            y = torch.randint(-2048, 2048, (images, H // up, W // up, cpad), dtype=torch.int16, device="cuda")
        args = (x, 4, y, 4, up, first, 4, True, 4, False)
        _native.add_up_resident(*args)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            _native.add_up_resident(*args)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) / iters * 1e3
        nbytes = x.numel() * (1 + (2 if first else 0) + 1) + y.numel() * y.element_size()
        rows.append(("%s %s + %s -> %s" % (name, "int8", "int8" if first else "int16", "wide + narrow" if first else "narrow"), us,
                     nbytes, nbytes / us / 1e3))
    return rows


def time_steps(net, x, iters):
    """Per top-down step: the device time of its lateral convolution, upsampling, add and output convolution, summed, median
    over `iters` forwards (a deferred convolution launches inside the add that runs it, so the sum holds either way)."""
    marks, hooks = {}, []

    def pre(mod, inp, n):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.setdefault(n, []).append([e])

    def post(mod, inp, out, n):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks[n][-1].append(e)

    for _label, names in STEPS:
        for n in names:
            m = net.get_submodule(n)
            hooks.append(m.register_forward_pre_hook(lambda mod, inp, n=n: pre(mod, inp, n)))
            hooks.append(m.register_forward_hook(lambda mod, inp, out, n=n: post(mod, inp, out, n)))
    with torch.no_grad():
        for _ in range(iters):
            net(x)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    out = []
    for label, names in STEPS:
        per_iter = [sum(marks[n][i][0].elapsed_time(marks[n][i][1]) for n in names) for i in range(iters)]
        out.append((label, float(np.median(per_iter)) * 1e3))
    return out


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
    say("model: ResNet-50-FPN, really calibrated, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0, "the logits are constant"
        if key == arms[0]:
            shapes = add_shapes(net, a.images)
        plan = resident.enable(net, x, concat=True, topdown=True) if key == "on" else resident.enable(net, x, concat=True)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident logits differ from the plain forward (%s)" % key
        logits[key] = (out, plain)
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d" % (key, plan["fp32_outputs"]))
        for name, why in sorted(resident.describe(net).topdown_left.items()):
            say("  left as it was: %s: %s" % (name, why))
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
    say("the top-down steps one by one (lateral convolution + upsampling + add + output convolution, device time, median of %d forwards):"
        % max(a.iters, 5))
    for key in arms:
        for label, us in time_steps(nets[key], x, max(a.iters, 5)):
            say("  %-3s %-28s %9.1f us" % (key, label, us))
    say("fq_add_up_resident alone at the model's launch shapes (back-to-back launches, device events; bytes moved / time, and that as "
        "a share of %.0f TB/s):" % (HBM_GBS / 1e3))
    for (label, us, nbytes, gbs) in time_kernel(shapes, a.images):
        say("  %-52s %8.1f us  %8.2f MB  %7.0f GB/s  %5.1f %%" % (label, us, nbytes / 1e6, gbs, 100.0 * gbs / HBM_GBS))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
