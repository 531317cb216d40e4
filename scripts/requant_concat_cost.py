"""What the re-quantising Concat is worth inside a network: the resident int8-sim forward of two really calibrated models,
resident.enable(net, x, concat=True, bilinear=True) against resident.enable(net, x, concat=True, bilinear=True, requant=True), in
one process, alternating, timed with device events.

    python scripts/requant_concat_cost.py [--arms both|off|on] [--models unet,resunet] [--images 64] [--size 224] [--rounds 5]
                                          [--iters 10] [--seed 0] [--out FILE]

  unet      model/unet/UNet_fabu.py, UNet(base_width 32, depth 4): the model of scripts/bilinear_cost.py, whose record is 2 of 4
            upsamplings planned (two revoked because their Concat's reader sits on another bit than its skip)
  resunet   model/unet/ResUNet_fabu.py at its defaults: every Concat joins the int16 sum of a stage with a bilinear upsampling

Each model is seeded, its batch norms folded (merge_bn) and it is really calibrated on the GPU on two batches of 16 seeded images.
Each arm's resident output is checked against its plain forward and against the other arm's; its plan summary (`fp32_outputs`,
`resident_concats`, `resident_bilinears`, `requant_concats`, `requant_sum_sources`) and what describe().bilinear_left /
.requant_left name are printed -- whatever is still left is shown with its reason --, then every round times `iters` forwards of
each arm; a line per round, the median and spread of each arm and the median on / off ratio.  Last, fq_concat_rq_i8_nhwc alone is
timed at the launch shapes the on arm recorded -- back-to-back launches between device events -- alternating with
fq_concat_n_i8_nhwc (the nearest mover) at the same output shape with int8 sources: bytes moved, GB/s, the share of the HBM's
8 TB/s, the ratio of the two and whether the working set fits the 256 MiB Infinity Cache.  For int8-only sources the two move the
same bytes; an int16 source adds its second byte.
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
L3_BYTES = 256 << 20
OFF = dict(concat=True, bilinear=True)
ON = dict(concat=True, bilinear=True, requant=True)


def build_model(kind, a, device):
    from common.quantity import merge_bn
    torch.manual_seed(a.seed)
    if kind == "unet":
        from model.unet.UNet_fabu import UNet
        model = UNet(num_classes=2, input_size=a.size, base_width=32, depth=4)
    else:
        from model.unet.ResUNet_fabu import ResUNet
        model = ResUNet(num_classes=2, input_size=a.size)
    g = torch.Generator().manual_seed(a.seed)
    with torch.no_grad():
        for name, p in model.named_parameters():            # He-style spread for the weights; the batch norms keep gamma 1
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / max(1, p[0].numel())) ** 0.5)
            elif name.endswith("bias"):                     # (a folded bias of exactly zero has no weight bit)
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return merge_bn(model.eval()).to(device)


def build_nets(kind, a, arms):
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.size, a.size), torch.cuda.current_device())      # cwd = its test/ directory
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(16, 3, a.size, a.size, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(kind, a, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(kind, a, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s_%s.pth" % (kind, key))
    return nets, tmp


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


def time_kernels(launches, iters=200, rounds=5):
    """The re-quantising kernel and the mover at the recorded launches, alternating over `rounds`."""
    from common.quantity import _native
    rows = []
    for launch in launches:                                 # [(source shape, dtype, C, up, relu, shift), ...]
        srcs, plain = [], []
        for shape, dtype, c, up, relu, shift in launch:
            lim = 100 if dtype == torch.int8 else 3000
            srcs.append((torch.randint(-lim, lim, shape, dtype=dtype, device="cuda"), c, up, relu, shift))
            plain.append((torch.randint(-100, 100, shape, dtype=torch.int8, device="cuda"), c, up, relu))
        n, h, w = launch[0][0][0], launch[0][0][1] * launch[0][3], launch[0][0][2] * launch[0][3]
        out = torch.empty(n, h, w, _native.pad16(sum(s[2] for s in launch)), dtype=torch.int8, device="cuda")
        rq, mv = [], []
        for _ in range(rounds):
            rq.append(_per_launch(lambda: _native.concat_rq_i8_nhwc(srcs, out=out), iters))
            mv.append(_per_launch(lambda: _native.concat_n_i8_nhwc(plain, out=out), iters))
        b_rq = sum(s[0].numel() * s[0].element_size() for s in srcs) + out.numel()
        b_mv = sum(s[0].numel() for s in plain) + out.numel()
        label = "[%d, %d, %d] " % (n, h, w) + " + ".join("%d ch int%d shift %d" % (c, 8 * torch.empty(0, dtype=d).element_size(), sh)
                                                            for _s, d, c, _u, _r, sh in launch)
        rows.append((label, float(np.median(rq)), float(np.median(mv)), (max(rq) - min(rq)) / float(np.median(rq)),
                     (max(mv) - min(mv)) / float(np.median(mv)), b_rq, b_mv))
    return rows


def run_model(kind, a, arms, say):
    from common.quantity import _native, resident
    nets, tmp = build_nets(kind, a, arms)
    say("model %s: seed %d, really calibrated, %d images at %d x %d, arms %s" % (kind, a.seed, a.images, a.size, a.size, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.size, a.size)).astype(np.float32)).cuda()
    outs, launches = {}, []
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0, "the output is constant"
        plan = resident.enable(net, x, **(ON if key == "on" else OFF))
        real = _native.concat_rq_i8_nhwc
        if key == "on":
            _native.concat_rq_i8_nhwc = lambda srcs, **k: (launches.append([(tuple(s[0].shape), s[0].dtype, int(s[1]), int(s[2]), bool(s[3]), int(s[4]))
                                                                            for s in srcs]), real(srcs, **k))[1]
        try:
            with torch.no_grad():
                out = net(x)
        finally:
            _native.concat_rq_i8_nhwc = real
        assert torch.equal(out, plain), "resident output differs from the plain forward (%s, %s)" % (kind, key)
        outs[key] = (out, plain)
        say("%s %s: plan %s" % (kind, key, dict(sorted(plan.items()))))
        say("%s %s: fp32_outputs %d, resident_concats %d, resident_bilinears %d, requant_concats %s, requant_sum_sources %s"
            % (kind, key, plan["fp32_outputs"], plan["resident_concats"], plan["resident_bilinears"], plan.get("requant_concats", "-"),
               plan.get("requant_sum_sources", "-")))
        d = resident.describe(net)
        for name, why in sorted(d.bilinear_left.items()):
            say("  bilinear_left: %s: %s" % (name, why))
        for name, why in sorted(d.requant_left.items()):
            say("  requant_left: %s: %s" % (name, why))
    if len(arms) == 2:
        assert torch.equal(outs["off"][0], outs["on"][0]) and torch.equal(outs["off"][1], outs["on"][1]), "the two arms disagree"
        say("%s outputs: on == off == plain forward" % kind)
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
        say("%s round %d: " % (kind, r) + ", ".join("%s %.3f ms" % (k, ms[k]) for k in arms) + " per %d-image forward" % a.images
            + (", ratio on / off %.3f" % (ms["on"] / ms["off"]) if len(arms) == 2 else ""))
    for key in arms:
        v = per_arm[key]
        say("%s %s: median %.3f ms, min %.3f, max %.3f, spread (max - min) / median %.3f, %.0f images/s"
            % (kind, key, float(np.median(v)), min(v), max(v), (max(v) - min(v)) / float(np.median(v)), a.images / float(np.median(v)) * 1e3))
    if len(arms) == 2:
        say("%s median ratio on / off: %.3f" % (kind, float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])]))))
    del nets, outs
    torch.cuda.empty_cache()
    if launches:
        say("%s: fq_concat_rq_i8_nhwc alone at the on arm's launches, next to fq_concat_n_i8_nhwc at the same output shape with int8 "
            "sources (back-to-back launches, device events, medians of 5 alternating rounds; share of %.0f TB/s):" % (kind, HBM_GBS / 1e3))
        for (label, us_r, us_m, sp_r, sp_m, b_r, b_m) in time_kernels(launches):
            say("  %-58s requant %8.1f us %7.0f GB/s %5.1f %% (spread %.3f) | mover %8.1f us %7.0f GB/s (spread %.3f) | time ratio %.3f, "
                "byte ratio %.3f | %8.2f MB, %s"
                % (label, us_r, b_r / us_r / 1e3, 100.0 * b_r / us_r / 1e3 / HBM_GBS, sp_r, us_m, b_m / us_m / 1e3, sp_m, us_r / us_m,
                   b_r / float(b_m), b_r / 1e6, "fits the Infinity Cache" if b_r <= L3_BYTES else "larger than the Infinity Cache"))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--models", default="unet,resunet")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    a.out = os.path.abspath(a.out) if a.out else None      # (build_nets changes the working directory)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                           # (kept up to date: a run that is cut short leaves what it measured)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for kind in a.models.split(","):
        assert kind in ("unet", "resunet"), kind
        run_model(kind, a, arms, say)


if __name__ == "__main__":
    main()
