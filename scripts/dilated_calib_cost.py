#!/usr/bin/env python3
"""What the atrous dense fp32 kernel (fq_conv_dil_f32) costs and saves on one GPU.

  --arms both|off|on   DeepLabV3 (model/deeplab/DeepLabV3_fabu.py, ResNet-50, BatchNorm merged) calibrated in two passes with
                       Quantity.own_dilated off / on, arms alternating in one process over --rounds rounds: median [min .. max] per
                       arm, the own launch counts, and whether feat.table is identical; then the FIRST calibration of a fresh
                       child process per arm (--first), the arms alternating over --fresh children each
  --probe              fq_conv_dil_f32 (abs-max and ReLU copy in the epilogue) alone at each distinct dilated launch shape of the
                       model at --batch images, alternating with what it replaces (the library convolution without bias, then the
                       bias-add producer with the abs-max and the ReLU copy): median [min .. max] of --iters launches each, HOST-timed with a
                       synchronisation per launch (enqueue and sync are inside the figure: it is no kernel time), the live
                       products per host-timed second as a share of the fp32 MFMA peak (157.3 TFLOP/s), and the live taps per tile
Run from the repository root after build():   python scripts/dilated_calib_cost.py --probe [--output-stride 8] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))                     # cases.py: the seeded models and batches of the tests

import torch  # noqa: E402
from torch import nn  # noqa: E402

PEAK = 157.3e12


def spread(ts):
    return "%.3f [%.3f .. %.3f] ms" % (statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def live_taps(h, w, d, pad, th, tw):
    """live taps per tile of a TH x TW tiling, averaged over the tiles of a plane (the rule of fq_conv_dil_f32_geom.h)"""
    ho, wo = h + 2 * pad - 2 * d, w + 2 * pad - 2 * d
    def axis(o0, ln, L):
        return sum(1 for r in range(3) if max(o0 - pad + r * d, 0) < min(o0 - pad + r * d + ln, L))
    tiles = [(axis(p, min(th, ho - p), h), axis(q, min(tw, wo - q), w)) for p in range(0, ho, th) for q in range(0, wo, tw)]
    return sum(a * b for a, b in tiles) / len(tiles)


def probe(model, args, say):
    from common.quantity import _native
    shapes, hooks = {}, []

    def note(mod, i, o):
        shapes.setdefault((mod.in_channels, mod.out_channels, i[0].shape[2], i[0].shape[3], mod.dilation[0], mod.padding[0]), mod)
    for m in model.modules():
        if isinstance(m, nn.Conv2d) and m.groups == 1 and m.dilation[0] > 1:
            hooks.append(m.register_forward_hook(note))
    with torch.no_grad():
        model(torch.zeros(1, 3, args.size, args.size, device="cuda"))
    for h in hooks:
        h.remove()
    for (cin, cout, h, w, d, pad), m in shapes.items():
        x = torch.randn(args.batch, cin, h, w, device="cuda")
        wq, mx, relu = _native.pack_kxk_weight(m.weight), torch.zeros(1, device="cuda"), None
        y = _native.conv_dil_f32(x, wq, m.bias, d, pad)
        relu = torch.empty_like(y)
        own = lambda: _native.conv_dil_f32(x, wq, m.bias, d, pad, max_dev=mx, row=0, relu_out=relu, out=y)

        def lib():
            with torch.no_grad():
                v = m._conv_forward(x, m.weight, None)
                _native.bias_add_absmax(v, m.bias, mx, 0, relu_out=relu)
        t_own, t_lib = [], []
        for _ in range(3):                                                        # arms alternate
            t_own += timed(own, args.iters)
            t_lib += timed(lib, args.iters)
        tw = min(w, 32)
        th = min(h, 128 // tw)
        lt = live_taps(h, w, d, pad, th, tw)
        live_flops = 2.0 * args.batch * cout * h * w * cin * sum(
            1 for p in range(h) for q in range(w) for r in range(3) for s in range(3)
            if 0 <= p - pad + r * d < h and 0 <= q - pad + s * d < w) / (h * w)
        say("  %4d -> %4d  %2dx%-2d d %2d: own %s | library + bias producer %s | ratio %.2f | live products per host-timed second: %.1f %% of "
            "the MFMA peak | %.2f live taps per tile" % (cin, cout, h, w, d, spread(t_own), spread(t_lib),
                                                    statistics.median(t_own) / statistics.median(t_lib),
                                                    100.0 * live_flops / statistics.median(t_own) / PEAK, lt))


def calibrate(model, batches, own):
    from tools import Quantity
    from workdir_util import product_workdir
    with product_workdir(input_shape="1,3,%d,%d" % (batches[0][0].shape[2], batches[0][0].shape[3]), device="gpu",
                         max_cali_img_num=len(batches) - 1) as tmp:
        q = Quantity(model)
        q.own_dilated = own
        torch.cuda.synchronize()
        t = time.perf_counter()
        q.activation_quantize(batches)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        return dt, open(tmp + "/test/workdir/feat.table", "rb").read(), q.timings["own_conv1x1_launches"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arms", choices=("both", "off", "on"), default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--output-stride", type=int, default=16)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--fresh", type=int, default=2, help="fresh child processes per arm")
    ap.add_argument("--first", action="store_true", help="one calibration of the arm given, timed, nothing else (the child process)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    import cases
    from common.quantity import merge_bn
    from model.deeplab.DeepLabV3_fabu import DeepLabV3
    model = merge_bn(cases.seed_model(DeepLabV3(output_stride=args.output_stride, width=args.width, input_size=args.size)).eval()).cuda()
    say("DeepLabV3 (ResNet-50, width %d) at output stride %d, %d x %d, %s" % (args.width, args.output_stride, args.size, args.size,
                                                                             torch.cuda.get_device_name(0)))
    if args.first:
        batches = cases.calib_batches(args.images // args.batch, (args.batch, 3, args.size, args.size), seed=31)
        print("FIRST %.3f" % calibrate(model, batches, args.arms == "on")[0], flush=True)
        return
    if args.probe:
        say("fq_conv_dil_f32 alone against what it replaces, N = %d:" % args.batch)
        probe(model, args, say)
    else:
        batches = cases.calib_batches(args.images // args.batch, (args.batch, 3, args.size, args.size), seed=31)
        arms = {"both": (False, True), "off": (False,), "on": (True,)}[args.arms]
        times, tables, counts = {a: [] for a in arms}, {}, {}
        for rnd in range(args.rounds + 1):                                        # round 0 warms both arms up and is not counted
            for a in arms:
                dt, tables[a], counts[a] = calibrate(model, batches, a)
                if rnd == 0:
                    say("  warm-up calibration of this process (off before on: no first-use comparison), own_dilated %s: %.3f s"
                        % ("on" if a else "off", dt))
                else:
                    times[a].append(dt)
        for a in arms:
            say("  own_dilated %-3s: %s per calibration, %d own launches" % ("on" if a else "off", spread(times[a]), counts[a]))
        if len(arms) == 2:
            rows = list(zip(tables[False].splitlines(), tables[True].splitlines()))
            say("  ratio on / off %.3f; feat.table rows that differ: %d of %d" % (
                statistics.median(times[True]) / statistics.median(times[False]), sum(a != b for a, b in rows), len(rows)))
        firsts = {a: [] for a in arms}
        for _ in range(args.fresh):                                               # a fresh process per arm and turn: its first calibration
            for a in arms:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--first", "--arms", "on" if a else "off", "--images",
                                      str(args.images), "--batch", str(args.batch), "--size", str(args.size), "--output-stride",
                                      str(args.output_stride), "--width", str(args.width)], capture_output=True, text=True, timeout=300)
                got = [ln for ln in out.stdout.splitlines() if ln.startswith("FIRST ")]
                if not got:
                    raise SystemExit("the child process failed: " + out.stderr[-400:])
                firsts[a].append(float(got[0].split()[1]))
        for a in arms:
            say("  fresh process, own_dilated %-3s: first calibration %s s" % ("on" if a else "off", ", ".join("%.3f" % v for v in firsts[a])))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
