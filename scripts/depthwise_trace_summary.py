"""Per-layer reading of two rocprofv3 kernel traces of scripts/depthwise_cost.py (one run with --arms on, one with --arms off):
for every depthwise layer of the MobileNet-shaped model, the time of fq::dwconv_i8_kernel, its algorithmic bytes (int8 input +
int8 output + weights, from the layer shapes) over that time as a share of 8 TB/s, and the summed time of the launches the off
arm spends on the same layer between the two pointwise kernels around it.

    python scripts/depthwise_trace_summary.py --on DIR_ON/..._kernel_trace.csv --off DIR_OFF/..._kernel_trace.csv [--images 256] [--variant v1]

A forward is cut out of a trace at the classifier's kernel (linear_i8_wave_kernel); only forwards with one depthwise segment per
layer are used (the calibration's and the plan's traced forwards differ), the median over them is printed.  In the on arm the
n-th fq::dwconv_i8_kernel of a forward is layer n.  In the off arm the integer convolution kernels delimit segments, and a
segment that holds the Quantity kernel of the reference-shaped form is a depthwise layer: Quantity, the library's grouped fp32
convolution, the tail, the ReLU and the next layer's quantise + repack.  Needs no GPU.
"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 8.0
INFINITY_CACHE = 256 << 20


def layer_shapes(variant, images, hw=224):
    """(name, C, kernel, stride, H, P, bytes) per depthwise layer, from the architecture table of the model file."""
    sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))
    from model.mobilenet import MobileNet_fabu as mf
    rows, width, h = [], mf.STEM_WIDTH, hw // 2
    for n, (out, stride) in enumerate(mf.BLOCKS):
        k = 5 if (variant == "residual" and out == mf.LAST_STAGE_WIDTH) else 3
        p = (h + 2 * (k // 2) - k) // stride + 1
        cpad = (width + 15) // 16 * 16
        rows.append(("blocks.%d.dw.0" % n, width, k, stride, h, p, images * (h * h + p * p) * cpad + k * k * cpad))
        width, h = out, p
    return rows


def forwards(path):
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out, cur = [], []
    for r in rows:
        cur.append((r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        if "linear_i8_wave_kernel" in r["Kernel_Name"]:
            out.append(cur)
            cur = []
    return out


def is_integer_conv(name):
    return name.startswith("void fq::") and any(k in name for k in ("conv2d_i8", "conv1x1_i8", "conv3x3_i8", "stem_conv_i8",
                                                                     "block_tail", "linear_i8"))


def on_layers(fwd):
    return [us for name, us in fwd if "dwconv_i8_kernel" in name]


def off_layers(fwd):
    """[(summed microseconds, launches)] of the segments between integer convolution kernels that hold a Quantity kernel."""
    out, seg, started = [], [], False
    for name, us in fwd:
        if is_integer_conv(name):
            if started and any("QuantityOp" in n for n, _ in seg):
                out.append((sum(u for _, u in seg), len(seg)))
            seg, started = [], True
        else:
            seg.append((name, us))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--on", required=True)
    ap.add_argument("--off", required=True)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--variant", choices=["v1", "residual"], default="v1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = layer_shapes(a.variant, a.images)
    on = [v for v in (on_layers(f) for f in forwards(a.on)) if len(v) == len(shapes)]
    off = [v for v in (off_layers(f) for f in forwards(a.off)) if len(v) == len(shapes)]
    assert on and off, "no complete forward found (on: %d, off: %d)" % (len(on), len(off))
    lines = ["forwards used: on %d, off %d; %d images; time in microseconds, median over the forwards" % (len(on), len(off), a.images),
             "%-16s %5s %4s %2s %9s %9s %9s %7s %6s %5s %10s %9s %7s" % ("layer", "C", "k", "s", "HxH", "PxP", "MB", "on us", "TB/s",
                                                                          "%HBM", "off us", "launches", "off/on")]
    tot_on = tot_off = 0.0
    for i, (name, C, k, s, h, p, nbytes) in enumerate(shapes):
        t_on = statistics.median(v[i] for v in on)
        t_off = statistics.median(v[i][0] for v in off)
        n_off = off[-1][i][1]
        tbs = nbytes / (t_on * 1e-6) / 1e12
        tot_on, tot_off = tot_on + t_on, tot_off + t_off
        lines.append("%-16s %5d %dx%d %2d %4dx%-4d %4dx%-4d %9.2f %7.1f %6.2f %5.0f %10.1f %9d %7.1f%s"
                     % (name, C, k, k, s, h, h, p, p, nbytes / 1e6, t_on, tbs, 100 * tbs / HBM_TBS, t_off, n_off, t_off / t_on,
                        "   (input + output fit the 256 MiB Infinity Cache)" if nbytes < INFINITY_CACHE else ""))
    lines.append("all depthwise layers: on %.1f us, off %.1f us per forward" % (tot_on, tot_off))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
