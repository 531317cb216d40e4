"""What the atrous depthwise int8 kernel is worth inside a network: the resident int8-sim forward of DeepLabV3+ on MobileNetV2
(model/deeplab/DeepLabV3Plus_fabu.py) under resident.enable(net, x, depthwise=True, relu6=True, concat=True, flatten=True,
bilinear=True, requant=True), with NewConv2d.use_atrous_i8 off against on, in one process, alternating, timed with device events.

    python scripts/atrous_cost.py [--arms both|off|on] [--images 64] [--size 224] [--output-stride 16] [--width 1.0]
                                  [--rounds 5] [--iters 10] [--seed 0] [--probe] [--out FILE]

The model is seeded, its batch norms folded (merge_bn) and it is really calibrated on the GPU on two batches of 16 seeded images
(activation_quantize, weight_quantize; SUPPORT_DILATION on: the weights of the dilated layers are quantised as they are).
Reconstruction builds one ReconModel per arm; the on arm sets use_atrous_i8 on its own layers.  Each arm's resident logits are
checked against its plain forward and against the other arm's, the plan summaries (`fp32_outputs`, `resident_depthwise`) are
printed, then every round times `iters` forwards of each arm; a line per round, the median and spread of each arm and the median
on / off ratio.  --probe: per dilated launch shape of the model, fq_dwconv2d_dil_i8_resident alone (back-to-back launches between
device events, medians of 5 alternating rounds) next to the DENSE depthwise kernel at the same tensor shape with d = 1 and
padding 1 -- the same bytes in and out, so that is the yardstick -- with the share of a phase tile's columns that hold an output.
"""
import argparse
import os
import shutil
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SWITCHES = dict(depthwise=True, relu6=True, concat=True, flatten=True, bilinear=True, requant=True)


def build_model(a, device):
    from common.quantity import merge_bn
    from model.deeplab.DeepLabV3Plus_fabu import DeepLabV3Plus
    torch.manual_seed(a.seed)
    model = DeepLabV3Plus(num_classes=21, output_stride=a.output_stride, width_mult=a.width, input_size=a.size)
    g = torch.Generator().manual_seed(a.seed)
    with torch.no_grad():
        for name, p in model.named_parameters():            # He-style spread for the weights; the batch norms keep gamma 1
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / max(1, p[0].numel())) ** 0.5)
            elif name.endswith("bias"):                     # (a folded bias of exactly zero has no weight bit)
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return merge_bn(model.eval()).to(device)


def build_nets(a, arms):
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.size, a.size), torch.cuda.current_device())      # cwd = its test/ directory
    path = os.path.join(tmp, "tools", "configs.yml")
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    cfg["SETTINGS"]["SUPPORT_DILATION"] = True
    with open(path, "w") as fh:
        yaml.safe_dump(cfg, fh)
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(16, 3, a.size, a.size, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(a, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(a, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s.pth" % key)
    return nets, tmp


def dilated_shapes(net, x):
    """(N, H, W, C, R, d, pad) -> number of layers, of every dilated depthwise layer's input, from one hooked forward."""
    from common.quantity import NewConv2d
    rows, hooks = {}, []

    def note(mod, inp, out):
        c, t = mod.Conv, inp[0]
        key = (int(t.shape[0]), int(t.shape[2]), int(t.shape[3]), c.in_channels, c.kernel_size[0], c.dilation[0], c.padding[0])
        rows[key] = rows.get(key, 0) + 1
    for m in net.modules():
        if isinstance(m, NewConv2d) and m.Conv.groups > 1 and m.Conv.dilation[0] > 1:
            hooks.append(m.register_forward_hook(note))
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return rows


def _per_launch(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def probe(shapes, say, iters=200, rounds=5):
    from common.quantity import _native
    say("fq_dwconv2d_dil_i8_resident alone at the model's dilated launch shapes, next to fq_dwconv2d_i8_resident at the same tensor "
        "shape with d = 1, padding 1 (back-to-back launches, device events, medians of %d alternating rounds of %d; bytes = 2 N H W "
        "Cpad; columns used = outputs / (4 * column tiles) of a line):" % (rounds, iters))
    for (n, h, w, c, r, d, pad), count in sorted(shapes.items()):
        cpad = _native.pad16(c)
        x = torch.randint(-128, 128, (n, h, w, cpad), dtype=torch.int8, device="cuda")
        wq = torch.randint(-128, 128, (r, r, cpad), dtype=torch.int8, device="cuda")
        qb = torch.zeros(c, device="cuda")
        dil, dense = [], []
        for _ in range(rounds):
            dil.append(_per_launch(lambda: _native.dwconv2d_dil_i8_resident(x, wq, qb, (pad, pad), (d, d), 7, 3, True), iters))
            dense.append(_per_launch(lambda: _native.dwconv2d_i8_resident(x, wq, qb, (1, 1), (r // 2, r // 2), 7, 3, True), iters))
        q_out = w + 2 * pad - d * (r - 1)
        tiles = min(d, q_out) * ((-(-q_out // d) + 3) // 4)
        md, ms, nbytes = float(np.median(dil)), float(np.median(dense)), 2 * n * h * w * cpad
        say("  [%d, %d, %d, %d] %dx%d d %2d (x%d): dilated %8.1f us (spread %.3f) %6.0f GB/s | dense %8.1f us (spread %.3f) %6.0f GB/s | "
            "dilated / dense %.2f | columns used %.2f%s"
            % (n, h, w, c, r, r, d, count, md, (max(dil) - min(dil)) / md, nbytes / md / 1e3, ms, (max(dense) - min(dense)) / ms,
               nbytes / ms / 1e3, md / ms, q_out / (4.0 * tiles), "  (Q < 4d)" if q_out < 4 * d else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--output-stride", type=int, default=16)
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from common.quantity import NewConv2d, resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, tmp = build_nets(a, arms)
    say("model: DeepLabV3Plus(output_stride %d, width_mult %.2f), seed %d, really calibrated, %d images at %d x %d, arms %s"
        % (a.output_stride, a.width, a.seed, a.images, a.size, a.size, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.size, a.size)).astype(np.float32)).cuda()
    outs, shapes = {}, {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0, "the output is constant"
        if key == arms[0]:
            shapes = dilated_shapes(net, x)
        dws = [m for m in net.modules() if isinstance(m, NewConv2d) and m.Conv.groups > 1]
        if key == "on":
            for m in dws:
                m.use_atrous_i8 = True
        plan = resident.enable(net, x, **SWITCHES)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident output differs from the plain forward (%s)" % key
        outs[key] = (out, plain)
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d, resident_depthwise %d of %d depthwise layers (%d dilated)"
            % (key, plan["fp32_outputs"], plan["resident_depthwise"], len(dws), sum(m.Conv.dilation[0] > 1 for m in dws)))
        for m in dws:
            if m.Conv.dilation[0] > 1 and m._atrous_left(m.Conv) is not None:
                say("  not taken: dilation %d: %s" % (m.Conv.dilation[0], m._atrous_left(m.Conv)))
    if len(arms) == 2:
        assert torch.equal(outs["off"][0], outs["on"][0]) and torch.equal(outs["off"][1], outs["on"][1]), "the two arms disagree"
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
    if a.probe:
        probe(shapes, say)
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
