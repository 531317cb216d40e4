"""What the transposed fp32 kernel (fq_deconv_f32) is worth inside the calibration (tools.Quantity.activation_quantize):
UNet(base_width 32, depth 4, up="deconv") of model/unet/UNet_fabu.py after merge_bn, up_kernel 2 and 4, 64 seeded images at
224 x 224 in batches of 16 that already live on the device, own_deconv off against on, alternating in one process after
Quantity.reserve_pool(), timed with the host clock around a synchronised call.

    python scripts/deconv_calib_cost.py [--arms both|off|on] [--images 64] [--batch 16] [--rounds 5] [--out FILE]

Per up_kernel: one untimed calibration per arm comes first (code load, the once-per-module checks, in the off arm the convolution
library's first-use search -- its time is printed: that search is what a fresh process pays); then every round times one
calibration of each arm; a line per round, the spread of each arm and the median on / off ratio are printed, and the tables of
the two arms are compared.

Then, per up-convolution of the model at the batch size of the calibration, the kernel alone (device events, median of 20 after 3
warm-up calls): the abs-max form and the histogram form of fq_deconv_f32 against what they replace with the switch off: the
library's transposed convolution (bias included) plus the separate statistic launch on its output (fq_absmax_seg /
fq_hist2048_seg).  Next to each the two bounds of DESIGN.md section 36: bytes of x + y over 8 TB/s and
2 N H W Cin Cout R S FLOP over 157 TFLOP/s.

`--arms off` never touches the new switch or the new entry point: this file copied into a checkout of the commit before the kernel
gives the baseline.
"""
import argparse
import os
import shutil
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def build_model(up_kernel, device):
    from common.quantity import merge_bn
    from model.unet.UNet_fabu import UNet
    torch.manual_seed(0)
    model = UNet(num_classes=2, input_size=224, base_width=32, depth=4, batch_norm=True, up="deconv", up_kernel=up_kernel)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def up_inputs(model, x):
    """(module, its input) of every up-convolution, from one hooked forward."""
    rows, hooks = [], []
    for m in model.ups:
        hooks.append(m.register_forward_hook(lambda mod, inp, out: rows.append((mod, inp[0].detach().clone()))))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return rows


def timed(fn, reps=20, warm=3):
    """Median and spread (min, max) of fn() in microseconds, device events."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def kernel_table(model, x, say, with_own):
    from common.quantity import _native as nat
    say("per up-convolution at N = %d (us: median [min, max] of 20): bounds = bytes of x + y over 8 TB/s, 2 N H W Cin Cout R S FLOP over 157 TFLOP/s"
        % x.shape[0])
    for m, xin in up_inputs(model, x):
        N, cin, H, W = xin.shape
        cout, (R, S), st, pd, op = m.out_channels, m.kernel_size, m.stride[0], m.padding[0], m.output_padding[0]
        with torch.no_grad():
            y = m(xin)
        mb = 4.0 * (xin.numel() + y.numel())
        flop = 2.0 * N * H * W * cin * cout * R * S
        say("  %d -> %d, %dx%d s%d p%d op%d, %dx%d -> %dx%d: %.1f MB = %.1f us at 8 TB/s, %.2f GFLOP = %.1f us at 157 TFLOP/s"
            % (cin, cout, R, S, st, pd, op, H, W, y.shape[2], y.shape[3], mb / 1e6, mb / 8e6, flop / 1e9, flop / 157e6))
        mx = torch.zeros(1, device="cuda")
        amax = float(y.abs().max())
        iv = torch.tensor([amax / 2048 + 1e-12], device="cuda")
        hist = torch.zeros(1, 2048, dtype=torch.int64, device="cuda")

        def lib_max():
            with torch.no_grad():
                o = m(xin)
            nat.absmax_seg([o], [0], mx)

        def lib_hist():
            with torch.no_grad():
                o = m(xin)
            nat.hist2048_seg([o], [0], iv, hist)

        def lib_alone():
            with torch.no_grad():
                m(xin)
        say("    library conv_transpose2d alone       %8.1f [%8.1f, %8.1f]" % timed(lib_alone))
        say("    library + fq_absmax_seg              %8.1f [%8.1f, %8.1f]" % timed(lib_max))
        say("    library + fq_hist2048_seg            %8.1f [%8.1f, %8.1f]" % timed(lib_hist))
        if not with_own:
            continue
        wt = m.weight.detach().permute(2, 3, 0, 1).reshape(R * S * cin, cout).contiguous()
        out = torch.empty_like(y)
        say("    fq_deconv_f32 abs-max form            %8.1f [%8.1f, %8.1f]"
            % timed(lambda: nat.deconv_f32(xin, wt, m.bias, (R, S), st, pd, op, max_dev=mx, row=0, out=out)))
        say("    fq_deconv_f32 histogram form          %8.1f [%8.1f, %8.1f]"
            % timed(lambda: nat.deconv_f32(xin, wt, m.bias, (R, S), st, pd, op, interval_dev=iv, hist_dev=hist, row=0, out=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    import bench
    from tools import Quantity
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    nb = a.images // a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    real_stdout = sys.stdout
    tmp = bench.make_workdir(nb - 1, "1,3,224,224", torch.cuda.current_device())     # cwd = its test/ directory
    rng = np.random.default_rng(99)
    batches = [(torch.from_numpy(rng.standard_normal((a.batch, 3, 224, 224)).astype(np.float32)).cuda(),
                torch.zeros(a.batch, dtype=torch.long)) for _ in range(nb)]
    for up_kernel in (2, 4):
        sys.stdout = open(os.devnull, "w")                                          # the drop-in prints like the reference does
        model = build_model(up_kernel, "cuda")
        sys.stdout = real_stdout
        say("model: UNet(base_width 32, depth 4, up='deconv', up_kernel %d), calibration of %d images at 224 x 224 in %d batches of %d, arms %s"
            % (up_kernel, nb * a.batch, nb, a.batch, arms))

        def calibrate(key):
            sys.stdout = open(os.devnull, "w")
            try:
                q = Quantity(model)
                if key == "on":
                    q.own_deconv = True
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q.activation_quantize(batches)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                sys.stdout = real_stdout
            return dt, q.timings, open("./workdir/feat.table").read()

        tables = {}
        for key in arms:                                                            # untimed: first use of everything
            dt, _tm, tables[key] = calibrate(key)
            say("%s: first calibration of the process %.3f s" % (key, dt))
        Quantity.reserve_pool()
        for key in arms:
            dt, tm, table = calibrate(key)
            assert table == tables[key], "feat.table of arm %s changed from one calibration to the next" % key
            say("%s: own_conv1x1_launches %s, fused_hist_launches %s, cached_batches %s, pass1 %.3f s, pass2 %.3f s"
                % (key, tm.get("own_conv1x1_launches"), tm.get("fused_hist_launches"), tm.get("cached_batches"), tm.get("pass1_s"),
                   tm.get("pass2_s")))
        if len(arms) == 2:
            ra, rb = tables["off"].splitlines(), tables["on"].splitlines()
            say("feat.table rows that differ between the arms: %d of %d" % (sum(u != v for u, v in zip(ra, rb)), len(ra)))
        per_arm = {key: [] for key in arms}
        for r in range(a.rounds):
            s = {}
            for key in arms:
                s[key], _tm, _t = calibrate(key)
                per_arm[key].append(s[key])
            say("round %d: " % r + ", ".join("%s %.4f s" % (k, s[k]) for k in arms) + " per %d-image calibration" % (nb * a.batch)
                + (", ratio on / off %.3f" % (s["on"] / s["off"]) if len(arms) == 2 else ""))
        for key in arms:
            v = per_arm[key]
            say("%s: median %.4f s, min %.4f, max %.4f, spread (max - min) / median %.3f"
                % (key, float(np.median(v)), min(v), max(v), (max(v) - min(v)) / float(np.median(v))))
        if len(arms) == 2:
            say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))
        kernel_table(model, batches[0][0], say, "on" in arms)
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
