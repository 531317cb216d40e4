#!/usr/bin/env python3
"""Headline benchmark: KL calibration throughput of a fabu ResNet-50 @224^2 on MI355X
(BASELINE.json metric "calibration images/sec + int8-sim images/sec", configs[1] at N=1).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Both forms work for N > 1: the bare form (no RANK in the environment) starts the second one as a CHILD process before anything
touches the GPU (spawn_ranks: free master port on 127.0.0.1, rank 0's JSON line relayed, the child's exit code returned; nothing
is re-exec'ed).  The line says what the collectives saw: `ranks_seen` (dist.get_world_size()), `backend`, and `devices`, one
(rank, device index, device name) entry per rank.

WORKLOAD.  K = --steps batches of 256 images PER GPU (--batch to change the size): the step is a fixed amount of work and
K sets how many are timed; the default 20 steps are BASELINE configs[1]'s "5k" (5 120 images).  `--images I` instead fixes
the images per GPU and cuts them into K batches (batch = ceil(I / K)).
`--total-images T` instead fixes the WHOLE job (strong scaling, "scaling": "strong"; `--gpus 8 --total-images 50000` is
BASELINE configs[3] verbatim): ceil(T / 256) batches of 256 images (--batch to change it) dealt round-robin to the ranks, the
SAME batch at every N -- so that the N = 1 and the N = 8 point of the curve time the same kernels -- and --steps is derived
(the batches of the busiest rank).  Every line carries expected_own_conv_launches / own_conv_launches: pass 1 must have run
every convolution of every owned batch on the own kernels; a rank that fell back to the library makes the bench exit 3.
A "step" is one calibration batch taken through the whole hot path: forward -> abs-max (pass 1), forward -> 2048-bin
histograms (pass 2); the timed region is ONE complete Quantity.activation_quantize() over the K batches of every GPU:
both passes, the MAX / SUM all-reduces, the KL threshold sweep of all 71 rows and the feat.table write.  Inputs are
synthetic fp32 images generated on the device BEFORE the timed region.  value = images processed by all ranks / wall
time (max over ranks, bracketed by barrier + synchronize); ms_per_step = that wall time / K.

A plain run does only that: set up, warm up, time the K steps and print the line (the headline keys, the workload, the
phases, feat_table_sha256 / statistics_sha256 and what the timed region's own HIP events measured: `roofline`,
`roofline_hist_chain`, `roofline_hist_pair`).  `--dump-outputs DIR` also writes what the timed calibration computed as
DIR/<name>.npy (rank 0, dump_outputs()); the same arguments give the same inputs, so two builds can be compared array by
array.  Everything else is measured with `--full` only (the --no-* switches select within it).

With --full the JSON line also carries
  value_cold   : the same workload in a FRESH process whose allocator pool is empty when the clock starts (no activation
                 cache: the engine never grows its pool for one; every hipMalloc inside the clock) -- what a one-shot
                 calibration script gets; `value` itself runs in a process that holds a warm pool (a long-running calibration service);
  roofline     : the dominant hand-written kernel (hist2048_seg), algorithmic bytes (4 B x elements per launch) / its
                 mean launch duration measured with HIP events on the launch stream inside the timed region;
                 `traffic` is STATIC (PMC counters of the committed profile of this configuration), and says so;
  roofline_bias_add_absmax / roofline_add_absmax : the two kernels pass 1's maxima ride on where the convolution itself
                 (fq_conv*_f32) or the one-kernel residual tail (below) does not take the statistic -- absent when none ran;
  roofline_conv1x1_add_f32 / roofline_conv1x1_add_hist_f32 : the last 1x1 convolution of a residual block + Eltwise + ReLU
                 in one kernel (pass 1 / pass 2): matrix work and algorithmic bytes (x, Wt, the shortcut, the ReLU output and
                 whichever of the two intermediate tensors is kept), frac_of_bound against max(matrix, bytes) per launch;
  file_input   : the same images as .npy files through PRE_PROCESS.IMG = 2 (--input-mode npy|both), beside `value`, never it
                 (the process's second such calibration, like `value`; first_run_images_per_s: the first, which page-locks its staging ring);
  roofline_conv_stem_f32 / roofline_conv_kxk_f32 : the same for the 7x7 stride-2 stem (fq_conv_stem_f32) and the stride-2 3x3
                 layers (fq_conv_kxk_f32); roofline_conv_wino_f32: the stride-1 3x3 layers (fq_conv3x3_wino_f32, Winograd);
  roofline_conv1x1_f32 : the float forward's 1x1 convolutions on the fp32 matrix cores (fq_conv1x1_f32, statistic in the
                 epilogue): 2 x MAC / summed launch durations against the 157.3 TFLOP/s dense fp32 MFMA peak;
  cpu_baseline : the CPU oracle (oracle/fq_oracle.c, "port") + torch-CPU forwards timed on a bounded sample on this
                 box's host cores at 1 thread and at all cores, scaled to the same workload (rank 0, N=1 only);
  (the forward-throughput keys below run --int8-batch images per forward, default 256)
  int8_sim_images_per_s : ReconModel forward throughput with resident integer activations (logits checked
                 bit-identical to the fp32-boundary model in the same run, see int8_sim_resident);
  int8_sim_fp32_boundary_images_per_s : the same ReconModel with the reference's fp32 NCHW module boundaries;
  int8_sim_hipgraph_images_per_s : the resident forward replayed as one HIP graph (input copy included);
  int8_sim_dual_graph_images_per_s : the same batch as two graphs of half the images replayed on two streams;
  roofline_int8_conv : 2 x MACs of the model / summed durations of the int8 conv launches of one resident forward
                 (HIP events), against the 5 000 TOP/s dense int8 MFMA peak;
  fakequant_images_per_s / float_forward_images_per_s : ReconTest and the float model;
  per_channel_calibration / roofline_per_channel : the per-(tensor, channel) extension.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
QUANTITY = os.path.join(ROOT, "pytorch-quantity_amd", "quantity")
sys.path.insert(0, QUANTITY)
sys.path.insert(0, ROOT)

with open(os.path.join(ROOT, "BASELINE.json")) as _fh:
    BASELINE_METRIC = json.load(_fh)["metric"]          # the reference's headline metric, verbatim
HBM_PEAK_GBS = 8000.0                        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
INT8_PEAK_TOPS = 5000.0                      # dense int8 MFMA peak (2 x the BF16 rate)
F32_MFMA_PEAK_TFLOPS = 157.3                 # dense fp32 MFMA peak (v_mfma_f32_32x32x2_f32; = the fp32 vector peak, MI355X_MICROARCH.md)


class DeviceBatches(object):
    """Sequence of (images, None) pairs indexed by GLOBAL batch index; only this rank's batches
    (i % world == rank) exist, pre-generated in HBM from generator seed 1234 + i.  A rank holds at most DISTINCT of them
    (39 GB at 256 images of 224^2): its k-th batch for k >= DISTINCT is its (k % DISTINCT)-th again, so that a long run
    (large --steps) does not have to fit all its inputs in HBM beside the pool."""
    DISTINCT = 256

    def __init__(self, total, batch, hw, rank, world, device, on_host=False):
        self._items = {}
        self._total = total
        owned = list(range(rank, total, world))
        for k, i in enumerate(owned):
            if k >= self.DISTINCT:
                self._items[i] = self._items[owned[k % self.DISTINCT]]
                continue
            g = torch.Generator(device=device).manual_seed(1234 + i)
            t = torch.randn(batch, 3, hw, hw, generator=g, device=device)
            self._items[i] = t.cpu() if on_host else t       # --host-inputs: pageable host memory

    def __len__(self):
        return self._total

    def __getitem__(self, i):
        return self._items[i], None

    def owned(self):
        return list(self._items.values())


def make_workdir(max_cali_img_num, input_shape, gpu):
    import yaml
    tmp = tempfile.mkdtemp(prefix="fq_bench_")
    os.makedirs(os.path.join(tmp, "tools"))
    os.makedirs(os.path.join(tmp, "test"))
    with open(os.path.join(QUANTITY, "tools", "configs.yml")) as fh:
        cfg = yaml.safe_load(fh)
    cfg["SETTINGS"]["MAX_CALI_IMG_NUM"] = max_cali_img_num
    with open(os.path.join(tmp, "tools", "configs.yml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    with open(os.path.join(QUANTITY, "test", "user_configs.yml")) as fh:
        ucfg = yaml.safe_load(fh)
    ucfg["MODEL"]["INPUT_SHAPE"] = input_shape
    ucfg["SETTINGS"]["DEVICE"] = "gpu"
    ucfg["SETTINGS"]["GPU"] = gpu
    with open(os.path.join(tmp, "test", "user_configs.yml"), "w") as fh:
        yaml.safe_dump(ucfg, fh)
    os.chdir(os.path.join(tmp, "test"))
    return tmp


def build_model(name, hw, device):
    from common.quantity import merge_bn
    from model.resnet.ResNet_fabu import ResNet50, ResNet101
    torch.manual_seed(0)
    model = (ResNet50 if name == "r50" else ResNet101)(input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    model.eval()
    model = merge_bn(model)
    return model.to(device)


# ----------------------------------------------------------------------------------------------------------------------
# collectives of the bench itself (the calibration's own two all-reduces live in common.quantity._collectives)
# ----------------------------------------------------------------------------------------------------------------------
def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def all_ok(local_ok, device=None):
    """True on every rank iff `local_ok` is true on every rank (one MIN all-reduce).  Every rank must call it: errors
    are never handled by skipping a collective -- a rank that failed locally reports it here and all ranks leave the
    section together."""
    dist = _dist()
    if dist is None:
        return bool(local_ok)
    t = torch.tensor([1 if local_ok else 0], dtype=torch.int32, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def run_section(fn, device=None):
    """Run rank-LOCAL work `fn()` (no collectives inside) and agree on the outcome: returns (ok_everywhere, result or
    None, repr of the local error or None)."""
    result, err = None, None
    try:
        result = fn()
    except Exception as e:           # local only; the agreement below is the collective
        err = repr(e)
    return all_ok(err is None, device), result, err


def share_tables(workdir, names=("feat.table", "weight.table")):
    """Quantity writes its tables on rank 0 only, into rank 0's own scratch directory; the other ranks need the text to
    rebuild the model (Reconstruction.get_quantity_information reads ./workdir/*.table).  Rank 0 broadcasts the files,
    every other rank writes them into ITS workdir.  A collective: every rank calls it."""
    dist = _dist()
    if dist is None:
        return
    rank = dist.get_rank()
    payload = [None]
    if rank == 0:
        payload = [{n: open(os.path.join(workdir, n)).read() for n in names if os.path.isfile(os.path.join(workdir, n))}]
    dist.broadcast_object_list(payload, src=0)
    if rank != 0:
        os.makedirs(workdir, exist_ok=True)
        for n, text in payload[0].items():
            with open(os.path.join(workdir, n), "w") as fh:
                fh.write(text)


class CallTimer(object):
    """Wraps a _native entry point and brackets every call with HIP events on the launch stream (torch's current
    stream is the stream the C ABI is handed).  bytes_fn(args, kwargs) -> algorithmic bytes of that launch."""

    def __init__(self, native, name, bytes_fn, flops_fn=None, form=None):
        self.native, self.name, self.bytes_fn, self.flops_fn, self.form = native, name, bytes_fn, flops_fn, form
        self.orig = getattr(native, name)
        self.events, self.bytes, self.flops, self.forms = [], [], [], []
        self.enabled = False

    def __enter__(self):
        def wrapped(*a, **k):
            if not self.enabled:
                return self.orig(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = self.orig(*a, **k)
            e1.record()
            self.events.append((e0, e1))
            self.bytes.append(float(self.bytes_fn(a, k)))
            if self.flops_fn is not None:
                self.flops.append(float(self.flops_fn(a, k)))
                self.forms.append(self.form or ("hist" if k.get("hist_dev") is not None else
                                                ("absmax" if k.get("max_dev") is not None else "plain")))
            return r
        setattr(self.native, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.native, self.name, self.orig)

    def summary(self):
        if not self.events:
            return None
        ms = np.array([a.elapsed_time(b) for a, b in self.events])
        by = np.array(self.bytes)
        return {"launches": int(len(ms)), "mean_ms": float(ms.mean()), "bytes_per_launch": float(by.mean()),
                "gbs": float(by.sum() / (ms.sum() * 1e-3) / 1e9)}


def _seg_bytes(a, k):
    return 4.0 * sum(int(t.numel()) for t in a[0])


def _chain_bytes(a, k):             # hist2048_chain_seg(chains, ...): every chain reads its head and its L conv3 outputs once
    return 4.0 * sum(int(head.numel()) * (1 + len(ys)) for head, ys, _ry, _rs in a[0])


def _pair_bytes(a, k):              # hist2048_pair_seg(a_tensors, b_tensors, ...): both operands once (+ the ReLU output when asked for)
    relus = a[6] if len(a) > 6 else k.get("relu_outs")
    return 4.0 * sum(int(t.numel()) * (2 + (1 if relus is not None and relus[i] is not None else 0)) for i, t in enumerate(a[0]))


def _bias_add_bytes(a, k):          # y += bias[c] in place (4 B read + 4 B written) (+ 4 B for the fused ReLU's copy)
    relu = k.get("relu_out") if "relu_out" in k else (a[4] if len(a) > 4 else None)
    return (8.0 + (4.0 if relu is not None else 0.0)) * int(a[0].numel())


def _add_bytes(a, k):               # z = x + y (8 B read + 4 B written) (+ 4 B for the fused ReLU's copy)
    relu = k.get("relu_out") if "relu_out" in k else (a[5] if len(a) > 5 else None)
    return (12.0 + (4.0 if relu is not None else 0.0)) * int(a[0].numel())


def _out_copies(k):                 # y and the ReLU copy; y itself is not written when only its ReLU is read (out=False)
    return (1 if k.get("out") is not False else 0) + (1 if k.get("relu_out") is not None else 0)


def _c1_shape(a, k):
    x, wt = a[0], a[1]
    s = int(k.get("stride", a[3] if len(a) > 3 else 1))
    return int(x.shape[0]), int(x.shape[1]), int(wt.shape[1]), (int(x.shape[2]) - 1) // s + 1, (int(x.shape[3]) - 1) // s + 1


def _c1_flops(a, k):                # conv1x1_f32(x, wt, bias, stride, ...): 2 x MAC
    n, cin, cout, ho, wo = _c1_shape(a, k)
    return 2.0 * n * cout * ho * wo * cin


def _c1_bytes(a, k):                # x read once, Wt, y written (+ the ReLU copy)
    n, cin, cout, ho, wo = _c1_shape(a, k)
    return 4.0 * (a[0].numel() + a[1].numel() + n * cout * ho * wo * _out_copies(k))


def _c1_add_bytes(a, k):            # conv1x1_add_f32(x, wt, bias, stride, res, ...): x, Wt and the shortcut read, the ReLU output
    n, cin, cout, ho, wo = _c1_shape(a, k)          # written, the convolution's output and the sum only when they are kept
    kept = (1 if k.get("out") is not None else 0) + (1 if k.get("sum_out") is not None else 0)
    return 4.0 * (a[0].numel() + a[1].numel() + n * cout * ho * wo * (2 + kept))


def _stem_shape(a, k):              # conv_stem_f32(x, wp, bias, cout, kernel, stride, pad, ...)
    x, cout, (r, s_), stride, pad = a[0], int(a[3]), a[4], int(a[5]), int(a[6])
    ho, wo = (int(x.shape[2]) + 2 * pad - r) // stride + 1, (int(x.shape[3]) + 2 * pad - s_) // stride + 1
    return int(x.shape[0]), int(x.shape[1]), cout, ho, wo, r * s_


def _stem_flops(a, k):
    n, cin, cout, ho, wo, taps = _stem_shape(a, k)
    return 2.0 * n * cout * ho * wo * cin * taps


def _stem_bytes(a, k):
    n, cin, cout, ho, wo, taps = _stem_shape(a, k)
    return 4.0 * (a[0].numel() + a[1].numel() + n * cout * ho * wo * _out_copies(k))


def _kxk_shape(a, k):               # conv_kxk_f32(x, wt, bias, kernel, stride, pad, ...)
    x, wt, (r, s_), stride, pad = a[0], a[1], a[3], int(a[4]), int(a[5])
    ho, wo = (int(x.shape[2]) + 2 * pad - r) // stride + 1, (int(x.shape[3]) + 2 * pad - s_) // stride + 1
    return int(x.shape[0]), int(x.shape[1]), int(wt.shape[1]), ho, wo, r * s_


def _kxk_flops(a, k):
    n, cin, cout, ho, wo, taps = _kxk_shape(a, k)
    return 2.0 * n * cout * ho * wo * cin * taps


def _kxk_bytes(a, k):
    n, cin, cout, ho, wo, taps = _kxk_shape(a, k)
    return 4.0 * (a[0].numel() + a[1].numel() + n * cout * ho * wo * _out_copies(k))


def _wino_shape(a, k):              # conv_wino_f32(x, u, bias, cout, ...): stride 1, pad 1, 3x3
    x = a[0]
    return int(x.shape[0]), int(x.shape[1]), int(a[3]), int(x.shape[2]), int(x.shape[3])


def _wino_flops(a, k):
    """The multiply-adds the kernel ISSUES: 16 per 2x2 output tile, input channel and output channel (a 7x7 plane has 4x4
    tiles).  The direct sum of the same layer is 2.25 x that on even planes (_wino_direct_flops)."""
    n, cin, cout, h, w = _wino_shape(a, k)
    return 2.0 * 16 * n * ((h + 1) // 2) * ((w + 1) // 2) * cin * cout


def _wino_direct_flops(a, k):
    n, cin, cout, h, w = _wino_shape(a, k)
    return 2.0 * n * cout * h * w * cin * 9


def _wino_bytes(a, k):
    n, cin, cout, h, w = _wino_shape(a, k)
    return 4.0 * (a[0].numel() + a[1].numel() + n * cout * h * w * _out_copies(k))


def mfma_f32_roofline(kernel, kt, note, form=None):
    """fp32 matrix-core roofline of the float 1x1 convolutions: 2 x MAC of all timed launches / their summed durations
    against the dense fp32 MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH.md); bound_ms = sum over the launches of
    max(matrix work at that peak, algorithmic bytes at 8 TB/s) -- the 64-channel layers of the first stage are HBM bound.
    form: only the launches of that epilogue ("absmax" = pass 1, "hist" = pass 2)."""
    keep = [i for i, f in enumerate(kt.forms) if form is None or f == form]
    if not keep:
        return None
    ms = np.array([kt.events[i][0].elapsed_time(kt.events[i][1]) for i in keep])
    fl, by = np.array(kt.flops)[keep], np.array(kt.bytes)[keep]
    ach = fl.sum() / (ms.sum() * 1e-3) / 1e12
    bound = np.maximum(fl / (F32_MFMA_PEAK_TFLOPS * 1e12), by / (HBM_PEAK_GBS * 1e9)) * 1e3
    return {"bound": "mfma", "kernel": kernel, "achieved": round(float(ach), 1), "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(float(ach) / F32_MFMA_PEAK_TFLOPS, 4), "launches": int(len(ms)), "mean_launch_ms": round(float(ms.mean()), 4),
            "algorithmic_flops_per_launch": float(fl.mean()), "algorithmic_bytes_per_launch": float(by.mean()),
            "hbm_gbs": round(float(by.sum() / (ms.sum() * 1e-3) / 1e9), 1), "bound_ms_per_launch": round(float(bound.mean()), 4),
            "frac_of_bound": round(float(bound.sum() / ms.sum()), 4),
            "launches_hbm_bound_at_peak": int((by / (HBM_PEAK_GBS * 1e9) > fl / (F32_MFMA_PEAK_TFLOPS * 1e12)).sum()), "note": note}


def hbm_roofline(kernel, s, extra=None):
    ach = s["bytes_per_launch"] / (s["mean_ms"] * 1e-3) / 1e9
    out = {"bound": "hbm", "kernel": kernel, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(ach / HBM_PEAK_GBS, 4), "launches": s["launches"], "mean_launch_ms": round(s["mean_ms"], 4),
           "algorithmic_bytes_per_launch": s["bytes_per_launch"]}
    out.update(extra or {})
    return out


def int8_conv_roofline(float_model, int8_net, batch, forwards=3):
    """MFMA-side roofline of the integer contraction (the one MFMA kernel on the path): 2 x MACs of every Conv2d / Linear
    of the model per forward / the summed durations of the int8 conv launches of the resident forward, HIP events on
    the launch stream around every C-ABI call.  Peak: 5 000 TOP/s dense int8 (2 x the BF16 MFMA rate, MI355X_MICROARCH.md)."""
    from common.quantity import _native
    macs, hooks = [0], []

    def count(m, i, o):
        w = m.weight
        macs[0] += int(o.numel()) * int(w[0].numel())                 # outputs x (C_in / groups x kh x kw)
    for m in float_model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            hooks.append(m.register_forward_hook(count))
    with torch.no_grad():
        float_model(batch)
    for h in hooks:
        h.remove()
    names = ("conv2d_i8_resident", "conv2d_i8_add_resident", "conv2d_i8_stem", "conv2d_i8", "block_tail_i8", "block_tail_proj_i8")
    events, saved = [], {n: getattr(_native, n) for n in names}
    bytes_of, macs_of = [], []

    def nbytes(*ts):
        return sum(int(t.numel()) * t.element_size() for t in ts if isinstance(t, torch.Tensor))

    def timed(fn, name):
        def wrapper(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            events.append((e0, e1))
            outs = r if isinstance(r, tuple) else (r,)
            # algorithmic traffic of the launch: activation operand + weights + (fused add) residual + everything written
            res = a[8] if name == "conv2d_i8_add_resident" else (a[5] if name == "block_tail_i8" else None)
            # fq_block_tail_i8 also runs the next block's 1x1 reduction: its weights, its matrix work, its int8 output
            w_next = (a[12] if len(a) > 12 else k.get("w1q")) if name == "block_tail_i8" else None
            w_proj = None
            if name == "block_tail_proj_i8":                      # ... and the projection shortcut: its input, weights, matrix work
                res, w_proj = a[5], a[6]                           # (xp is what is read in place of the shortcut tensor)
                w_next = a[16] if len(a) > 16 else k.get("w1q")
            bytes_of.append(nbytes(a[0], a[1], res, w_next, w_proj, *outs))
            first = next(t for t in outs if isinstance(t, torch.Tensor))
            pixels = first.numel() // first.shape[1 if first.dtype == torch.float32 else -1]
            wq = a[1]                                              # [K][R][S][Cpad] (stem: [R][64][32])
            macs_of.append(pixels * (int(wq.numel()) + (int(w_next.numel()) if w_next is not None else 0)
                                     + (int(w_proj.numel()) if w_proj is not None else 0)))
            return r
        return wrapper
    try:
        for n in names:
            setattr(_native, n, timed(saved[n], n))
        with torch.no_grad():
            for _ in range(forwards):
                int8_net(batch)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(_native, n, saved[n])
    per = [a.elapsed_time(b) for a, b in events]
    ms = sum(per) / forwards
    achieved = 2.0 * macs[0] / (ms * 1e-3) / 1e12
    # what the semantics allow: every launch costs at least its matrix work at the int8 peak AND its operand / result
    # traffic at the HBM peak (the exact int16 residual stream of the reference's fp32 adds is most of the bytes)
    n_l = len(events) // forwards
    t_mfma = [2.0 * m / (INT8_PEAK_TOPS * 1e12) * 1e3 for m in macs_of[:n_l]]
    t_hbm = [b / (HBM_PEAK_GBS * 1e9) * 1e3 for b in bytes_of[:n_l]]
    bound_ms = sum(max(a, b) for a, b in zip(t_mfma, t_hbm))
    return {"bound": "mfma", "kernel": "conv2d_i8 / conv2d_i8_dma / conv3x3_i8_halo* / block_tail_i8 / stem_conv_i8 (all integer conv + linear "
                                       "launches of one forward)",
            "achieved": round(achieved, 1), "peak": INT8_PEAK_TOPS, "unit": "TOP/s", "frac": round(achieved / INT8_PEAK_TOPS, 4),
            "launches_per_forward": n_l, "ms_per_forward": round(ms, 4), "images_per_forward": int(batch.shape[0]),
            "gmac_per_image": round(macs[0] / int(batch.shape[0]) / 1e9, 3),
            "bound_ms_per_forward": round(bound_ms, 4), "frac_of_bound": round(bound_ms / ms, 4),
            "mfma_floor_ms": round(sum(t_mfma), 4), "hbm_floor_ms": round(sum(t_hbm), 4),
            "algorithmic_gb_per_forward": round(sum(bytes_of[:n_l]) / 1e9, 3),
            "launches_hbm_bound_at_peak": sum(1 for a, b in zip(t_mfma, t_hbm) if b > a),
            "note": "frac = 2 x MAC / time against the 5 POP/s int8 peak.  bound_ms = sum over the launches of max(matrix work at that "
                    "peak, algorithmic bytes at 8 TB/s): the exact int16 residual stream (5 B per output element of every conv3 + "
                    "NewAdd: the reference adds un-quantised fp32 values) makes most launches HBM bound -- frac_of_bound is the "
                    "fraction of what the semantics allow (DESIGN.md 5b)"}


def cpu_baseline(model_cpu_ctor, hw, n_images_full, q, log):
    """Bounded CPU run of the same workload: torch-CPU forward (what the reference does) + the CPU oracle for abs-max /
    histogram / KL, at ONE thread and at all host cores (<= 32), each scaled to the full image count.  Reported, not a
    target."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import fq_oracle as orc
    orc.build()
    model = model_cpu_ctor()
    names = ["image"] + list(q.net_info.keys())
    feats, hooks = {}, []
    state = {"n": 0}
    cared = set(q.net_info.keys())

    def hook(m, i, o):
        if state["n"] == 0:
            feats.clear()
            feats["image"] = i[0]
        state["n"] += 1
        k = "%s_%i" % (type(m).__name__, state["n"])
        if k in cared:
            feats[k] = o
        if state["n"] >= q.layers_num:
            state["n"] = 0

    for m in model.modules():
        if type(m).__name__ in q._all_op_type:
            hooks.append(m.register_forward_hook(hook))

    def measure(cores, sample_images, chunk=8):
        """The two-pass calibration of `sample_images` images on `cores` threads, `chunk` images per forward: pass 1 (forward +
        abs-max of every row), intervals, pass 2 (forward again + 2048-bin histograms), then one KL sweep of all rows."""
        torch.set_num_threads(cores)
        pool = ThreadPoolExecutor(cores)
        x = torch.randn(sample_images, 3, hw, hw, generator=torch.Generator().manual_seed(1234))
        with torch.no_grad():
            model(x[:1])                                                 # untimed: oneDNN primitive creation
        t0 = time.perf_counter()
        maxs = {n: 0.0 for n in names}
        for c0 in range(0, sample_images, chunk):                        # pass 1
            with torch.no_grad():
                model(x[c0:c0 + chunk])
            arrs = {n: feats[n].numpy().ravel() for n in names}
            for n, v in zip(names, pool.map(lambda n: orc.absmax(arrs[n]), names)):
                maxs[n] = max(maxs[n], v)
        ivs = {n: orc.interval(maxs[n]) for n in names}
        hists = {}
        for c0 in range(0, sample_images, chunk):                        # pass 2
            with torch.no_grad():
                model(x[c0:c0 + chunk])
            arrs = {n: feats[n].numpy().ravel() for n in names}
            for n, h in zip(names, pool.map(lambda n: orc.hist2048(arrs[n], ivs[n]), names)):
                hists[n] = h if n not in hists else hists[n] + h
        t_img = (time.perf_counter() - t0) / sample_images
        t1 = time.perf_counter()
        list(pool.map(lambda n: orc.kl_threshold(orc.normalize(hists[n])), names))
        t_kl = time.perf_counter() - t1
        pool.shutdown()
        log("cpu_baseline[%d threads]: %.3f s/image over %d images (2 forwards + absmax + hist), KL %.2f s for %d tensors"
            % (cores, t_img, sample_images, t_kl, len(names)))
        return {"value": round(n_images_full / (n_images_full * t_img + t_kl), 3), "cores": cores,
                "s_per_image": round(t_img, 4), "kl_sweep_s": round(t_kl, 3), "sample_images": sample_images}

    many = min(os.cpu_count() or 1, 32)          # beyond one socket's worth oneDNN only gets slower
    one = measure(1, 2)
    full = measure(many, 32)
    for h in hooks:
        h.remove()
    return {"value": full["value"], "unit": "images/s", "cores": full["cores"], "kind": "port",
            "single_thread": {"value": one["value"], "unit": "images/s", "cores": 1, "s_per_image": one["s_per_image"],
                              "kl_sweep_s": one["kl_sweep_s"]},
            "all_cores": full,
            "sample": "%d images (all cores) / %d images (1 thread) through torch-CPU forward x2 + oracle absmax/hist2048, "
                      "+ one oracle KL sweep of all %d rows; scaled to %d images" % (full["sample_images"], one["sample_images"],
                                                                                     len(names), n_images_full)}


def dump_outputs(out_dir, q, bits):
    """--dump-outputs: what the timed calibration handed back and the statistics it was decided on, one row per tensor in the
    calibration's order ("image" first, then the cared layers, as in feat.table):
      bits.npy      float64[T]     the bit of every tensor, what activation_quantize() returns (feat.table is written from it);
      absmax.npy    float32[T]     the running abs-max after pass 1 (and its MAX all-reduce);
      hist.npy      float64[T, B]  the histogram counts after pass 2 (and its SUM all-reduce), exact as float64;
      threshold.npy float64[T]     the KL threshold of every tensor, (t* + 0.5) x its bin width."""
    names = list(q._quantizer._tensor_list)
    arrays = {"bits": np.array([bits[n] for n in names], dtype=np.float64),
              "absmax": q._collector.max_device.cpu().numpy().astype(np.float32),
              "hist": q._collector.hist_device.cpu().numpy().astype(np.float64),
              "threshold": np.array([q._quantizer.threshold_value[n] for n in names], dtype=np.float64)}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ----------------------------------------------------------------------------------------------------------------------
def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=0,
                    help="calibration images PER GPU (weak scaling), cut into --steps batches; default: --steps x --batch "
                         "(20 x 256 = BASELINE configs[1]'s 5k)")
    ap.add_argument("--total-images", type=int, default=0,
                    help="calibration images of the WHOLE job (strong scaling; overrides --images): "
                         "--gpus 8 --total-images 50000 is BASELINE configs[3]")
    ap.add_argument("--batch", type=int, default=0, help="images per step; default: 256, or --images / --steps")
    ap.add_argument("--model", default="r50", choices=["r50", "r101"])
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--host-inputs", action="store_true",
                    help="hand the calibrator pageable HOST batches (PCIe-inclusive rate; never the headline value)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-recon", action="store_true")
    ap.add_argument("--no-cold", action="store_true", help="skip the fresh-process run behind value_cold")
    ap.add_argument("--cold-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--int8-batch", type=int, default=256,
                    help="images per forward of the int8-sim / fake-quant throughput section")
    ap.add_argument("--no-per-channel", action="store_true")
    ap.add_argument("--allow-library-convs", action="store_true",
                    help="do not fail when convolutions of the timed region ran on the library instead of the own kernels")
    ap.add_argument("--input-mode", default="both", choices=["tensor", "npy", "both"],
                    help="tensor: device-resident batches only (the headline); npy / both: also the same images as one .npy file "
                         "each through PRE_PROCESS.IMG = 2 (reported as file_input, never the headline)")
    ap.add_argument("--no-file-input", action="store_true")
    ap.add_argument("--dry-launch", action="store_true",
                    help="launch plumbing only (no GPU needed): every rank joins a gloo group and rank 0 prints a JSON line with "
                         "ranks_seen / devices / the workload split -- what tests/test_bench_launch_cpu.py runs")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline as well: the fresh-process run (value_cold), the split-bf16 calibration, the "
                         "producer / fake-quant rooflines, the int8-sim / fake-quant / float forwards, the CPU baseline, file inputs "
                         "and the per-channel calibration (a plain run sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed calibration computed (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)          # the bench changes its working directory
    world = max(args.gpus, 1)
    if args.total_images:
        # STRONG scaling (BASELINE configs[3]): the whole job is fixed and so is the batch -- 256 images per forward at EVERY N, so that
        # t_1 and t_N time the same kernels on the same launch shapes (a batch derived from images / steps would run 2 500 images
        # per forward at N = 1, past the own convolutions' 2^30-element limit and onto the library).  The job is
        # ceil(total / batch) batches dealt round-robin; --steps is DERIVED: the batches the busiest rank owns.
        if args.batch <= 0:
            args.batch = 256
        args.total_batches = -(-args.total_images // args.batch)
        args.steps = -(-args.total_batches // world)
    else:
        # WEAK scaling: a step is one batch of a fixed size (256 unless --batch says otherwise), so that --steps sets how much
        # work is timed and ms_per_step is the time of the same unit of work at any K; --images I instead fixes the images
        # per GPU and cuts them into K batches.
        if args.batch <= 0:
            args.batch = max(1, -(-args.images // max(args.steps, 1))) if args.images else 256
        args.total_batches = args.steps * world
    args.scaling = "strong" if args.total_images else "weak"
    args.images_per_gpu = args.batch * args.steps            # the busiest rank's share (== --images when steps divides it)
    return args


def cold_child(args):
    """Fresh process, N = 1: (1) the very first activation_quantize() of the process, nothing warmed up at all (code loading and
    the once-per-module checks inside the clock): `one_shot_images_per_s`; (2) the allocator pool handed
    back to the driver (empty_cache), then the same workload again: every hipMalloc inside the clock, no activation
    cache (the engine never grows its pool for one), code and MIOpen warm: `value_cold`.  Prints one JSON line."""
    sys.stdout.flush()
    stdout_fd = os.dup(1)
    os.dup2(os.open(os.devnull, os.O_WRONLY), 1)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    from common.quantity import _native
    from tools import Quantity
    _native.lib()
    K, B, HW = args.steps, args.batch, args.image
    shape = "1,3,%d,%d" % (HW, HW)
    real_stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
    model = build_model(args.model, HW, device)
    data = DeviceBatches(K, B, HW, 0, 1, device)
    out = {}
    for tag in ("one_shot", "cold"):
        make_workdir(K - 1, shape, 0)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        reserved0 = torch.cuda.memory_reserved()
        q = Quantity(model)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.activation_quantize(data)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[tag] = {"images_per_s": round(K * B / dt, 1), "seconds": round(dt, 4),
                    "reserved_before_gb": round(reserved0 / 2 ** 30, 2),
                    "max_reserved_gb": round(torch.cuda.max_memory_reserved() / 2 ** 30, 1),
                    "cache_bytes": q.timings.get("cache_bytes"), "cache_plan": q.timings.get("cache_plan"),
                    "pass1_s": round(q.timings["pass1_s"], 4), "pass2_s": round(q.timings["pass2_s"], 4)}
        del q
    sys.stdout = real_stdout
    os.dup2(stdout_fd, 1)
    print(json.dumps(out), flush=True)


def run_cold_child(args, log):
    cmd = [sys.executable, os.path.abspath(__file__), "--cold-child", "--gpus", "1", "--steps", str(args.steps),
           "--batch", str(args.batch), "--model", args.model, "--image", str(args.image)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "FQ_ACT_CACHE_GB")}
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": "cold child rc %d: %s" % (r.returncode, r.stderr[-400:])}
        line = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")][-1]
        out = json.loads(line)
        out["process_wall_s"] = round(time.perf_counter() - t0, 1)
        log("cold child:", out)
        return out
    except Exception as e:
        return {"error": repr(e)}


def spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (the form the driver uses for N = 1): start
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py <same arguments>` as a CHILD process on a free
    port of 127.0.0.1, relay rank 0's JSON line and return the child's exit code.  This parent never touches the GPU
    (torch.cuda.device_count() does not initialise HIP on this stack) and nothing is exec'ed over a process that did."""
    import socket
    backend = os.environ.get("FQ_BENCH_BACKEND", "nccl")
    if not args.dry_launch and backend == "nccl" and torch.cuda.device_count() < args.gpus:
        print("bench.py --gpus %d: this node shows %d GPU(s).  (A dry run of the %d-rank flow on fewer devices: "
              "FQ_BENCH_BACKEND=gloo -- ranks then share devices and the number is not a scaling measurement.)"
              % (args.gpus, torch.cuda.device_count(), args.gpus), file=sys.stderr, flush=True)
        return 2
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    print("bench.py: starting %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)          # stderr is inherited: the ranks' logs stay visible
    lines = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
    if lines:
        print(lines[-1], flush=True)
    elif r.returncode == 0:
        print("bench.py: the ranks exited with 0 but printed no JSON line", file=sys.stderr, flush=True)
        return 1
    return r.returncode


def dry_launch(args):
    """--dry-launch: the launch plumbing without a GPU.  Every rank joins a gloo group, the ranks gather what each of them
    would bind to, and rank 0 prints the one JSON line -- same keys as the real line where they do not need a measurement."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    devices = [(rank, None, "cpu (dry launch)")]
    if "RANK" in os.environ:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        gathered = [None] * dist.get_world_size()
        dist.all_gather_object(gathered, devices[0])
        devices, world = gathered, dist.get_world_size()
        dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": BASELINE_METRIC, "dry_launch": True, "value": None, "unit": "images/s", "n_gpus": args.gpus,
                          "ranks_seen": world, "backend": "gloo", "devices": [list(d) for d in devices], "steps": args.steps,
                          "warmup": args.warmup, "scaling": args.scaling,
                          "config": {"batch": args.batch, "images_per_gpu": args.images_per_gpu,
                                     "images_total": args.total_batches * args.batch, "batches_total": args.total_batches,
                                     "parallelism": "dp%d" % world}}), flush=True)
    if "RANK" in os.environ:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    args = parse_args()
    if args.cold_child:
        return cold_child(args)
    if args.gpus > 1 and "RANK" not in os.environ:
        return spawn_ranks(args)
    if args.dry_launch:
        return dry_launch(args)

    # stdout carries exactly ONE line, the JSON.  Native libraries write there too (RCCL prints a version
    # banner on init), so file descriptor 1 itself is parked on /dev/null until the result is ready.
    sys.stdout.flush()
    stdout_fd = os.dup(1)
    null_fd = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null_fd, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench.py: --gpus %d but the launcher started %d ranks (WORLD_SIZE)" % (args.gpus, world), file=sys.stderr, flush=True)
        return 2

    def log(*a):
        if rank == 0:
            print(*a, file=sys.stderr, flush=True)

    # the fresh-process run goes FIRST, before this process touches the GPU: it needs the device's memory to itself
    cold = None
    if args.full and world == 1 and not args.no_cold and not args.host_inputs:
        cold = run_cold_child(args, log)

    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # one process per GPU.  (Dry run of the N > 1 flow on a single-GPU box: FQ_BENCH_BACKEND=gloo lets two ranks share
    # device 0 -- RCCL refuses duplicate devices -- with FQ_BENCH_POOL_FRAC sizing each rank's warm pool.)
    backend = os.environ.get("FQ_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    import torch.distributed as dist
    distributed = "RANK" in os.environ and "WORLD_SIZE" in os.environ      # launched by torch.distributed.run
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)              # backend nccl = RCCL on ROCm
        else:
            dist.init_process_group(backend)

    # what the collectives see (the driver's scaling run reads these: RCCL must have seen N ranks on N different devices)
    ranks_seen = dist.get_world_size() if distributed else 1
    devices = [(rank, dev_index, torch.cuda.get_device_name(dev_index))]
    if distributed:
        gathered = [None] * ranks_seen
        dist.all_gather_object(gathered, devices[0])
        devices = gathered
    sharing = max(sum(1 for d in devices if d[1] == dev_index), 1)            # ranks on this device (> 1 only in the gloo dry run)

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    torch.backends.cudnn.benchmark = os.environ.get("FQ_BENCH_MIOPEN_FIND", "0") == "1"   # MIOpen find mode: see DESIGN.md
    from common.quantity import _native
    from tools import Quantity, Reconstruction
    _native.lib()
    # every call of the segmented histogram since the process started, so that a kernel trace of this command can be cut to the
    # timed region's launches by position (roofline.trace_slice; scripts/summarize_profile.py writes them out one per row)
    hist_calls = [0]
    _hist_entry = _native.hist2048_seg

    def _counted_hist(*a, **k):
        hist_calls[0] += -(-len(a[0]) // 96)          # dispatches: fq_hist2048_seg takes 96 segments per launch (kSegChunk)
        return _hist_entry(*a, **k)
    _native.hist2048_seg = _counted_hist

    K, W, B, HW = args.steps, args.warmup, args.batch, args.image
    TB = args.total_batches                                # batches of the WHOLE job (weak: K per rank; strong: fixed, dealt i % world)
    n_owned = len(range(rank, TB, world))                  # ... of which this rank runs these (K on the busiest rank)
    shape = "1,3,%d,%d" % (HW, HW)
    devnull = open(os.devnull, "w")
    real_stdout = sys.stdout
    sys.stdout = devnull                                   # the drop-in prints like the reference does (merge_bn too):
    model = build_model(args.model, HW, device)            # stdout must carry exactly one JSON line

    # ---- warmup: W batches per GPU through the same path (MIOpen first-use solver search, RCCL init, code load)
    if W > 0:
        make_workdir(W * world - 1, shape, dev_index)
        warm = DeviceBatches(W * world, B, HW, rank, world, device)
        wq = Quantity(model)
        wq.activation_quantize(warm)
        del warm
        # Size the caching allocator's pool for the device before the clock starts: 80 % of HBM (288 GB per MI355X),
        # as a long-running calibration service would hold it.  The timed region then keeps pass 1's activations for
        # pass 2 in that pool (phases_s.cache_bytes) instead of paying 10-30 ms per GB of fresh hipMalloc; what a cold
        # one-shot process gets (no cache: the engine never grows its pool for one; allocation inside the clock) is
        # `value_cold`.
        if "FQ_ACT_CACHE_GB" not in os.environ:
            frac = float(os.environ.get("FQ_BENCH_POOL_FRAC", "%.4f" % (0.80 / sharing if sharing == 1 else 0.40 / sharing)))
            Quantity.reserve_pool(frac, device)           # the product's service-mode switch (tools.Quantity.reserve_pool)
        del wq
    barrier()

    # ---- timed: K batches per GPU
    make_workdir(TB - 1, shape, dev_index)
    data = DeviceBatches(TB, B, HW, rank, world, device, on_host=args.host_inputs)
    q = Quantity(model)
    q.profile_phases = True
    cache_budget = q._activation_cache_budget()            # per rank: every rank budgets its own GPU's pool
    hist_calls_before = hist_calls[0]
    with CallTimer(_native, "hist2048_seg", _seg_bytes) as kt_hist, CallTimer(_native, "hist2048_chain_seg", _chain_bytes) as kt_chain, \
            CallTimer(_native, "hist2048_pair_seg", _pair_bytes) as kt_pair:
        kt_hist.enabled = kt_chain.enabled = kt_pair.enabled = True
        barrier()
        t0 = time.perf_counter()
        bits = q.activation_quantize(data)
        barrier()
        elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if distributed:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    images = TB * B
    value = images / elapsed
    hist_s = kt_hist.summary()
    timings = dict(q.timings)
    timings["max_reserved_gb"] = round(torch.cuda.max_memory_reserved() / 2 ** 30, 1)
    timings["cache_budget_bytes_this_rank"] = int(cache_budget)
    feat_table = open("./workdir/feat.table").read() if rank == 0 else ""
    rows = len(q.net_info) + 1
    # Did the timed region stay on the own kernels?  Pass 1 runs every nn.Conv2d of every owned batch exactly once, either as its
    # own launch (own_conv1x1_launches) or inside its Eltwise's launch (conv_add_launches); a convolution that fell back to the
    # library (a tensor past the kernels' 2^30-element limit, a module that failed its check) is missing from that sum, and a
    # line with such a fallback inside is not comparable with one without -- every rank checks its own count, the ranks agree
    # (one MIN all-reduce), and the process exits non-zero.
    n_convs = sum(1 for m in model.modules() if type(m) is torch.nn.Conv2d)
    expected_own = n_convs * n_owned
    got_own = int(timings.get("own_conv1x1_launches", 0)) + int(timings.get("conv_add_launches", 0))
    own_everywhere = all_ok(got_own >= expected_own or args.allow_library_convs, device)

    result = {
        "metric": BASELINE_METRIC,
        "metric_note": "value = calibration images/s (both passes + KL sweep + feat.table, end to end) in SERVICE MODE: a process that "
                       "has calibrated before and holds a warm allocator pool of 80 % of HBM (230 GB), which pass 1's activations are kept "
                       "in for pass 2; with --full: value_cold = the same workload in a fresh process (allocation inside the clock); "
                       "int8-sim images/s is reported beside it as int8_sim_images_per_s (resident integer activations, logits "
                       "bit-identical to int8_sim_fp32_boundary_images_per_s, the reference's module-boundary form)",
        "value": round(value, 2), "unit": "images/s", "n_gpus": world, "ranks_seen": ranks_seen,
        "backend": (backend + (" (RCCL)" if backend == "nccl" else " (dry run: not RCCL)")) if distributed else "none (one process)",
        "devices": [list(d) for d in devices], "steps": K, "warmup": W,
        "ms_per_step": round(elapsed / K * 1e3, 3), "higher_is_better": True, "scaling": args.scaling,
        "vs_baseline": None, "dtype": "f32", "data": "synthetic" + (" (host-resident, PCIe inclusive)" if args.host_inputs else ""),
        "config": {"workload": "fabu ResNet-%s per-tensor KL calibration, %d synthetic 3x%dx%d images per GPU "
                               "(batch %d x %d steps), %d images in the whole job, %d histogram rows x 2048 bins" %
                               ("50" if args.model == "r50" else "101", K * B, HW, HW, B, K, images, rows),
                   "batch": B, "images_per_gpu": K * B, "images_total": images, "batches_total": TB,
                   "images_requested": args.total_images or (args.images or args.images_per_gpu) * world, "parallelism": "dp%d" % world,
                   "sharding": "batch i -> rank i %% %d; one MAX all-reduce of fp32[%d] after pass 1, one SUM all-reduce of "
                               "int64[%d] after pass 2 (RCCL); KL replicated; rank 0 writes feat.table" % (world, rows, rows * 2048),
                   "activation_cache": "pass-1 activations kept in a warm allocator pool (80 % of HBM, grown during warm-up); "
                                       "budgeted PER RANK from that rank's own pool (phases_s.cache_budget_bytes_this_rank), "
                                       "bytes used: phases_s.cache_bytes",
                   "int8_sim_images_per_forward": args.int8_batch},
        "phases_s": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in timings.items()},
        "expected_own_conv_launches": expected_own, "own_conv_launches": got_own,
        # what the calibration wrote (rank 0): integer sums and maxima are order independent, so the SAME job run on any number of
        # ranks must give the same digest -- bench.py --total-images T at N = 1 and N = 8 are comparable by this field
        "feat_table_sha256": __import__("hashlib").sha256(feat_table.encode()).hexdigest() if rank == 0 else None,
        # ... and what the table was made from: the 71 maxima and the 71 x 2048 histogram counts every rank holds after the two
        # all-reduces (the table's bits are a coarse function of them; this digest moves with a single count)
        "statistics_sha256": __import__("hashlib").sha256(q._collector.max_device.cpu().numpy().tobytes()
                                                          + q._collector.hist_device.cpu().numpy().tobytes()).hexdigest(),
        "own_conv_launches_note": "rank 0, pass 1: %d nn.Conv2d x %d owned batches must all have run on the own fp32-MFMA kernels "
                                  "(phases_s.own_conv1x1_launches + phases_s.conv_add_launches); every rank checks its own count and "
                                  "the bench exits 3 when any rank falls short" % (n_convs, n_owned),
    }
    if not own_everywhere:
        result["error"] = ("a rank's timed region left the own convolution kernels (expected %d launches on rank 0, saw %d): the line "
                           "is not comparable with the other points of the curve" % (expected_own, got_own))
    if cold is not None:
        if "cold" in cold:
            result["value_cold"] = cold["cold"]["images_per_s"]
            result["cold_process"] = {"what": "fresh process, N=1, same workload; value_cold: allocator pool empty when the clock "
                                              "starts (code warm from the process's first run), no activation cache; "
                                              "one_shot: the process's very first call, nothing warmed (code load, the once-per-module "
                                              "checks and allocation inside the clock; a calibration does not enter the convolution "
                                              "library)",
                                      "cold": cold["cold"], "one_shot": cold.get("one_shot"),
                                      "process_wall_s": cold.get("process_wall_s")}
        else:
            result["value_cold"] = None
            result["cold_process"] = cold
    traffic, traffic_src = None, None
    try:        # HBM bytes per launch from the PMC counters of the committed profile of this same configuration.  What a launch
        # covers depends on the cache plan, which follows the time stamps of the run's first forward: the committed entry
        # holds the measured RATIO of HBM bytes to algorithmic bytes, applied to this run's algorithmic bytes per launch.
        with open(os.path.join(ROOT, "profiles", "traffic_hist2048.json")) as fh:
            tj = json.load(fh)
        for ent in (tj if isinstance(tj, list) else [tj]):
            if (ent["batch"], ent["model"], ent["image"]) == (B, args.model, HW) and hist_s:
                ratio = ent["hbm_bytes_per_launch"] / ent["algorithmic_bytes_per_launch"]
                traffic = round(ratio * hist_s["bytes_per_launch"], 1)
                traffic_src = ("static: %.4f x this run's algorithmic bytes; the ratio is from %s (rocprofv3 --pmc of this "
                               "configuration, not measured in this run)" % (ratio, ent.get("source", "profiles/traffic_hist2048.json")))
                break
    except (OSError, KeyError, ValueError, ZeroDivisionError):
        pass
    if hist_s:
        result["roofline"] = hbm_roofline("hist2048_seg_kernel", hist_s, {"traffic": traffic, "traffic_source": traffic_src})
        # where the timed launches sit in a kernel trace of this command: dispatches [first, first + count) of hist2048_seg_kernel in
        # start order (a call is one dispatch per 96 segments; ResNet-50 has 71)
        result["roofline"]["trace_slice"] = {"kernel": "hist2048_seg_kernel", "first": hist_calls_before,
                                             "count": hist_calls[0] - hist_calls_before}

    # the residual stages' histograms of pass 2 (round 6): conv3 outputs and sums counted from (head, y_1 .. y_L) without any sum in HBM
    for key, kt, kernel, note in (
            ("roofline_hist_chain", kt_chain, "hist2048_chain_kernel<L>",
             "pass 2, one call per batch = one launch per residual stage (L = 3 / 4 / 6 / 3 blocks for ResNet-50): reads the stage's first "
             "shortcut and its L conv3 outputs once, counts 2 L rows, writes nothing; (L + 1) x 4 B per position"),
            ("roofline_hist_pair", kt_pair, "hist2048_pair_seg_kernel", "pass 2: a conv3 output and its sum from the pair (single blocks)")):
        sm = kt.summary()
        if sm:
            result[key] = hbm_roofline(kernel, sm, {"note": note, "launches_are": "calls of the entry point (a chain call launches one kernel per chain)"})

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, q, bits)

    def finish():
        sys.stdout = real_stdout
        sys.stdout.flush()
        os.dup2(stdout_fd, 1)
        if rank == 0:
            log("feat.table head:", feat_table.split("\n")[:4])
            print(json.dumps(result), flush=True)
        if distributed:
            barrier()
            dist.destroy_process_group()
        return 0 if own_everywhere else 3

    if not args.full:
        return finish()

    # ---- the same calibration with the float 1x1 layers on the split-bf16 kernels (FQ_CONV_SPLIT_BF16=1: every fp32 operand as three
    # bf16 pieces, six of the nine products on the bf16 matrix cores, fp32 accumulation -- as accurate as the fp32 fma chain, DESIGN.md
    # section 6c).  Off by default, so `value` above is the fp32-MFMA path; this is the opt-in path's number on the same batches.
    if world != 1:
        pass                                                    # (measured at N = 1; the key is absent from an N > 1 line)
    elif os.environ.get("FQ_BENCH_SPLIT_BF16", "1") == "0":
        result["split_bf16"] = {"skipped": "FQ_BENCH_SPLIT_BF16=0"}
    else:
        try:
            os.environ["FQ_CONV_SPLIT_BF16"] = "1"
            try:
                make_workdir(2 - 1, shape, dev_index)
                # packs the weights and runs every module's once-per-kernel check on the split-bf16 kernels, untimed
                Quantity(model).activation_quantize(DeviceBatches(2, B, HW, rank, world, device))
                make_workdir(TB - 1, shape, dev_index)
                sq = Quantity(model)
                sq.profile_phases = True
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                sq.activation_quantize(data)
                torch.cuda.synchronize(device)
                sb_elapsed = time.perf_counter() - t0
                result["split_bf16"] = {
                    "value": round(images / sb_elapsed, 2), "unit": "images/s", "seconds": round(sb_elapsed, 4),
                    "pass1_s": round(sq.timings.get("pass1_s", 0.0), 4), "pass2_s": round(sq.timings.get("pass2_s", 0.0), 4),
                    "same_table_as_value": open("./workdir/feat.table").read() == feat_table,
                    "what": "FQ_CONV_SPLIT_BF16=1: the 36 1x1 convolutions and the 16 residual tails of the float forward on "
                            "fq_conv1x1_sb_f32 / fq_conv1x1_sb_add_f32 / _add_hist_f32 instead of the fp32-MFMA kernels; same batches, same "
                            "warm pool; error against fp64 1.0-1.3e-7 of sum|w||x| (fp32 chain: 1.4-2.1e-7; profiles/r04_bf16x3_probe.txt)"}
                del sq
            finally:
                os.environ.pop("FQ_CONV_SPLIT_BF16", None)
                # what reads ./workdir next finds the headline run's table, not this section's
                make_workdir(TB - 1, shape, dev_index)
                os.makedirs("./workdir", exist_ok=True)
                with open("./workdir/feat.table", "w") as fh:
                    fh.write(feat_table)
        except Exception as e:
            result["split_bf16"] = {"error": repr(e)}

    # ---- pass 1's statistics ride on the producers' own kernels: their rooflines, measured on three more batches of
    # the same shape after the timed region (events around every one of the ~70 launches per forward would perturb it)
    # (one GPU only: the calibration below ends in the two all-reduces, and no collective may sit inside a try)
    try:
        if world != 1:
            raise RuntimeError("producer rooflines are measured at N = 1")
        with CallTimer(_native, "bias_add_absmax", _bias_add_bytes) as kt_b, CallTimer(_native, "add_absmax", _add_bytes) as kt_a, \
                CallTimer(_native, "bias_add_hist", _bias_add_bytes) as kt_bh, CallTimer(_native, "add_hist", _add_bytes) as kt_ah, \
                CallTimer(_native, "conv1x1_f32", _c1_bytes, _c1_flops) as kt_c1, \
                CallTimer(_native, "conv_stem_f32", _stem_bytes, _stem_flops) as kt_st, \
                CallTimer(_native, "conv_kxk_f32", _kxk_bytes, _kxk_flops) as kt_kk, \
                CallTimer(_native, "conv_wino_f32", _wino_bytes, _wino_flops) as kt_wi, \
                CallTimer(_native, "conv_wino_f32", _wino_bytes, _wino_direct_flops) as kt_wd, \
                CallTimer(_native, "conv1x1_add_f32", _c1_add_bytes, _c1_flops, "absmax") as kt_ca, \
                CallTimer(_native, "conv1x1_add_hist_f32", _c1_add_bytes, _c1_flops, "hist") as kt_cah:
            make_workdir(3 * world - 1, shape, dev_index)
            extra = DeviceBatches(3 * world, B, HW, rank, world, device)
            eq = Quantity(model)
            eq._activation_cache_budget = lambda: 0          # every batch through the second forward: all 69 producers fused
            kt_b.enabled = kt_a.enabled = kt_bh.enabled = kt_ah.enabled = kt_c1.enabled = kt_st.enabled = kt_kk.enabled = True
            kt_wi.enabled = kt_wd.enabled = True
            kt_ca.enabled = kt_cah.enabled = True
            eq.activation_quantize(extra)
            torch.cuda.synchronize()
            del extra, eq
        for key, kt, kernel, note in (
                ("roofline_bias_add_absmax", kt_b, "bias_add_absmax_kernel",
                 "pass 1, 53 launches per forward: y += bias[c] in place with max|y| (and the following ReLU's output) folded in; "
                 "8 B/element, 12 with the ReLU copy; mean over all layer sizes (the small late layers are launch bound)"),
                ("roofline_add_absmax", kt_a, "add_absmax_kernel",
                 "pass 1, 16 launches per forward: z = x + y with max|z| (and the ReLU's output) folded in; 12 B/element, 16 with "
                 "the ReLU copy"),
                ("roofline_bias_add_hist", kt_bh, "bias_add_hist_kernel",
                 "pass 2, the re-computed prefix of the network: y += bias[c] with the 2048-bin histogram of y (and the ReLU's "
                 "output) folded in; same algorithmic bytes as the pass-1 form"),
                ("roofline_add_hist", kt_ah, "add_hist_kernel", "pass 2: z = x + y with the histogram of z folded in")):
            sm = kt.summary()
            if sm:
                result[key] = hbm_roofline(kernel, sm, {"note": note, "aggregate_gbs": round(sm["gbs"], 1)})
        c1 = mfma_f32_roofline(
            "conv1x1_f32_absmax_kernel / conv1x1_f32_hist_kernel", kt_c1,
            "the float forward's 36 1x1 convolutions (2.12 of ResNet-50's 4.09 GMAC per image) on v_mfma_f32_32x32x2_f32 with the "
            "bias, the pass's statistic and the following ReLU in the epilogue: both passes of three batches, every layer size")
        if c1:
            # both forms together, then each: the abs-max form is what pass 1 (78 % of the timed region) runs; the histogram
            # form is a persistent grid of 2 workgroups per CU (8 KB of LDS bins on top of the three operand stages)
            for form in ("absmax", "hist"):
                part = mfma_f32_roofline("conv1x1_f32_%s_kernel" % form, kt_c1, None, form)
                if part:
                    c1["pass1_absmax_form" if form == "absmax" else "pass2_hist_form"] = {
                        k: part[k] for k in ("achieved", "frac", "launches", "mean_launch_ms", "frac_of_bound")}
            result["roofline_conv1x1_f32"] = c1
        for key, kt, kernel in (("roofline_conv1x1_add_f32", kt_ca, "conv1x1_f32_add_absmax_kernel"),
                                ("roofline_conv1x1_add_hist_f32", kt_cah, "conv1x1_f32_add_hist_kernel")):
            ca = mfma_f32_roofline(
                kernel, kt,
                "the last 1x1 convolution of each of the 16 residual blocks with the Eltwise that adds the shortcut and the ReLU behind "
                "it in the same kernel (both tensors' statistic in the epilogue; neither written when pass 2 keeps neither): 8 bytes "
                "per output element instead of the 20 the two kernels move; most of these launches are HBM bound even at the "
                "matrix peak, so read frac_of_bound and hbm_gbs, not frac")
            if ca:
                result[key] = ca
        stem = mfma_f32_roofline(
            "conv_stem_f32_absmax_kernel / conv_stem_f32_hist_kernel", kt_st,
            "the float forward's 7x7 stride-2 stem (0.118 GMAC per image) as an implicit GEMM on v_mfma_f32_32x32x2_f32, taps padded "
            "7 -> 8 (the flops counted are the 147 real taps), bias + statistic + ReLU in the epilogue; writes 2 x 822 MB per launch")
        if stem:
            result["roofline_conv_stem_f32"] = stem
        kk = mfma_f32_roofline(
            "conv1x1_f32_absmax_kernel<.., 2> / conv1x1_f32_hist_kernel<.., 2> (the R x S form of the same kernel)", kt_kk,
            "the float forward's 16 3x3 convolutions (1.85 GMAC per image) as direct convolutions on v_mfma_f32_32x32x2_f32: the "
            "1x1 kernel run tap by tap over shifted x rows, zero padding by select; both passes of three batches")
        if kk:
            for form in ("absmax", "hist"):
                part = mfma_f32_roofline("", kt_kk, None, form)
                if part:
                    kk["pass1_absmax_form" if form == "absmax" else "pass2_hist_form"] = {
                        k: part[k] for k in ("achieved", "frac", "launches", "mean_launch_ms", "frac_of_bound")}
            result["roofline_conv_kxk_f32"] = kk
        wi = mfma_f32_roofline(
            "wino_f32_absmax_kernel / wino_f32_hist_kernel", kt_wi,
            "the float forward's 13 stride-1 3x3 convolutions as Winograd F(2x2, 3x3) on v_mfma_f32_32x32x2_f32 (fq_conv3x3_wino_f32): "
            "16 products per 2x2 tile instead of 36, input and output transforms in the kernel.  achieved / frac count the "
            "multiply-adds the kernel issues (a 7x7 plane pays for 4x4 tiles); direct_equivalent_tflops is the direct sum's flop "
            "count over the same time -- what fq_conv_kxk_f32 would have to reach -- and may exceed the matrix peak")
        if wi:
            for form in ("absmax", "hist"):
                part = mfma_f32_roofline("", kt_wi, None, form)
                if part:
                    wi["pass1_absmax_form" if form == "absmax" else "pass2_hist_form"] = {
                        k: part[k] for k in ("achieved", "frac", "launches", "mean_launch_ms", "frac_of_bound")}
            wd = mfma_f32_roofline("", kt_wd, None)
            if wd:
                wi["direct_equivalent_tflops"] = wd["achieved"]
            result["roofline_conv_wino_f32"] = wi
    except Exception as e:
        if world == 1:
            result["roofline_bias_add_absmax"] = {"error": repr(e)}

    # ---- the fused fake-quant kernel on its own (north_star: >= 60 % of the HBM roofline).  EIGHT input / output pairs of 411 MB
    # each (6.6 GB) are walked round robin, so that no launch finds any of its bytes in the 256 MB Infinity Cache (one pair
    # replayed 20 times did: 822 MB is only 3.2 x the cache, and the fabric counters count its hits as traffic)
    try:
        n_el, pairs, reps = 802816 * 128, 8, 3                           # the largest ResNet-50 activation at batch 128
        xs = [torch.empty(n_el, device=device).normal_() for _ in range(pairs)]
        ys = [torch.empty(n_el, device=device) for _ in range(pairs)]
        for xq, yq in zip(xs, ys):
            _native.quandequan(xq, 4, 8, out=yq)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(pairs * reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            _native.quandequan(xs[i % pairs], 4, 8, out=ys[i % pairs])
            b.record()
        torch.cuda.synchronize()
        ms = float(np.mean([a.elapsed_time(b) for a, b in evs]))
        result["roofline_fakequant"] = hbm_roofline("unary_vec_kernel<QuanDequanOp>",
                                                    {"launches": len(evs), "mean_ms": ms, "bytes_per_launch": n_el * 8.0},
                                                    {"working_set_gb": round(pairs * n_el * 8.0 / 1e9, 2),
                                                     "note": "%d input/output pairs walked round robin (%.1f GB, 26 x the Infinity Cache): every "
                                                             "byte comes from / goes to HBM" % (pairs, pairs * n_el * 8.0 / 1e9)})
        del xs, ys
    except Exception as e:
        result["roofline_fakequant"] = {"error": repr(e)}
    # ... and the form ReconTest actually runs (TestConv.forward = convolution, then QuanDequan of its output, reference
    # new_quantity_op.py:283-292): the QuanDequan EPILOGUE of the own convolution kernels (conv1x1_f32_qd_kernel).  Measured on the
    # layer where the output stream dominates -- 64 -> 256 channels @56x56, 256 images: 205 MB read, 822 MB written, 26.3 GFLOP, so the
    # matrix pipe (0.167 ms at the fp32 MFMA peak) and HBM (0.128 ms at 8 TB/s) bound it about equally -- four operand sets round robin
    try:
        sets = 4
        xs = [torch.empty(256, 64, 56, 56, device=device).normal_() for _ in range(sets)]
        ys = [torch.empty(256, 256, 56, 56, device=device) for _ in range(sets)]
        wt = torch.empty(64, 256, device=device).normal_(0, 0.1)
        bq = torch.empty(256, device=device).normal_(0, 0.1)
        for xq, yq in zip(xs, ys):
            _native.conv1x1_f32(xq, wt, bq, 1, qd=(4, 8), out=yq)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(sets * 3)]
        for i, (a, b) in enumerate(evs):
            a.record()
            _native.conv1x1_f32(xs[i % sets], wt, bq, 1, qd=(4, 8), out=ys[i % sets])
            b.record()
        torch.cuda.synchronize()
        ms = float(np.mean([a.elapsed_time(b) for a, b in evs]))
        by = 4.0 * (xs[0].numel() + wt.numel() + ys[0].numel())
        fl = 2.0 * 256 * 56 * 56 * 64 * 256
        t_hbm, t_mfma = by / (HBM_PEAK_GBS * 1e9) * 1e3, fl / (F32_MFMA_PEAK_TFLOPS * 1e12) * 1e3
        result["roofline_fakequant_fused"] = {
            "bound": "mfma" if t_mfma >= t_hbm else "hbm", "kernel": "conv1x1_f32_qd_kernel (QuanDequan in the convolution's epilogue)",
            "layer": "64 -> 256 channels @56x56, 256 images", "launches": len(evs), "mean_launch_ms": round(ms, 4),
            "algorithmic_bytes_per_launch": by, "algorithmic_flops_per_launch": fl,
            "hbm_gbs": round(by / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "tflops": round(fl / (ms * 1e-3) / 1e12, 1), "frac_of_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
            "bound_ms_per_launch": round(max(t_hbm, t_mfma), 4), "frac_of_bound": round(max(t_hbm, t_mfma) / ms, 4),
            "working_set_gb": round(sets * by / 1e9, 2),
            "note": "what ReconTest runs: no standalone QuanDequan pass at all (4 B/element saved against convolution + fq_quandequan_f32)"}
        del xs, ys
    except Exception as e:
        result["roofline_fakequant_fused"] = {"error": repr(e)}

    # ---- int8-sim / fake-quant forward throughput (BASELINE config[2]); replicas only, no data-path collective.
    # Collectives in this section (barriers, the MAX of the elapsed times) are never inside a try: local work is
    # wrapped by run_section(), which ends in an agreement every rank takes part in.
    if not args.no_recon:
        ok, _, err = run_section(q.weight_quantize, device)              # rank 0 writes tables + JSON
        barrier()
        share_tables("./workdir")                                         # ... and every rank gets the two tables
        batches = [b.to(device) for b in data.owned()[:min(K, 8)]]
        if not batches:                                    # strong scaling with fewer batches than ranks: this rank owns none
            batches = [torch.randn(B, 3, HW, HW, generator=torch.Generator(device=device).manual_seed(99 + rank), device=device)]
        if args.int8_batch > B:                            # larger forwards: concatenated calibration batches
            per = (args.int8_batch + B - 1) // B
            src = batches if len(batches) >= per else batches * per
            batches = [torch.cat(src[i:i + per]) for i in range(0, len(src) - per + 1, per)][:4]
        elif args.int8_batch < B:
            batches = [b[:args.int8_batch] for b in batches[:4]]
        FB = int(batches[0].shape[0])

        def fwd_rate(net, passes=1):
            """images/s of net over the resident batches (None if any rank failed); the fast models take several
            passes so that one host hiccup (a GC pause is longer than a whole int8 forward) does not decide it."""
            err_local = None
            with torch.no_grad():
                try:
                    net(batches[0])
                except Exception as e:
                    err_local = repr(e)
                barrier()
                t0 = time.perf_counter()
                if err_local is None:
                    try:
                        for _ in range(passes):
                            for xb in batches:
                                net(xb)
                    except Exception as e:
                        err_local = repr(e)
                barrier()
            dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
            if distributed:
                dist.all_reduce(dt, op=dist.ReduceOp.MAX)
            if not all_ok(err_local is None, device):
                result.setdefault("recon_errors", []).append(err_local)
                return None
            return round(passes * len(batches) * FB * world / float(dt.item()), 1)

        if ok:
            result["float_forward_images_per_s"] = fwd_rate(model)

            def build_test():
                rec = Reconstruction(build_model(args.model, HW, device))
                return rec.ReconTest(rec.get_quantity_information(), "./workdir/recontest.pth")
            ok_t, test_net, err_t = run_section(build_test, device)
            if ok_t:
                result["fakequant_images_per_s"] = fwd_rate(test_net)
            del test_net

            def build_int8():
                rec2 = Reconstruction(build_model(args.model, HW, device))
                return rec2.ReconModel(rec2.get_quantity_information(), "./workdir/recon.pth")
            ok_i, int8_net, err_i = run_section(build_int8, device)
            if ok_i:
                result["int8_sim_fp32_boundary_images_per_s"] = fwd_rate(int8_net, 3)
                from common.quantity import resident

                def go_resident():
                    with torch.no_grad():
                        ref_logits = int8_net(batches[0])
                    plan = resident.enable(int8_net, batches[0])
                    _native.conv_variant_log = kernels = {}          # which integer-convolution kernels this forward launches
                    try:
                        with torch.no_grad():
                            same = bool(torch.equal(int8_net(batches[0]), ref_logits))
                    finally:
                        _native.conv_variant_log = None
                    plan = dict(plan, kernels=kernels)
                    return ref_logits, plan, same
                ok_r, res, err_r = run_section(go_resident, device)
                same_everywhere = ok_r and all_ok(res[2], device)
                if ok_r:
                    result["int8_sim_resident"] = {"bit_identical_logits": bool(res[2]), "plan": res[1], "images_per_forward": FB,
                                                   "checked_against": "the fp32-module-boundary form of the same model on the timed batch "
                                                                      "(torch.equal); the same dispatch (plan.kernels) against the reference's "
                                                                      "CPU logits: tests/test_gpu_r50_tables.py::test_r50_reconmodel_at_the_"
                                                                      "batch_the_bench_times_equals_the_reference"}
                if same_everywhere:                        # never report a rate for a model that computes something else
                    result["int8_sim_images_per_s"] = fwd_rate(int8_net, 8)
                    if rank == 0:
                        try:
                            result["roofline_int8_conv"] = int8_conv_roofline(model, int8_net, batches[0])
                        except Exception as e:
                            result["roofline_int8_conv"] = {"error": repr(e)}

                    def graph():
                        g = resident.capture(int8_net, batches[0])
                        with torch.no_grad():
                            if not torch.equal(g(batches[0]), res[0]):
                                raise RuntimeError("graph replay differs from the eager forward")
                            if len(batches) > 1 and not torch.equal(g(batches[1]), int8_net(batches[1])):
                                raise RuntimeError("graph replay on a second input differs from the eager forward")
                        return g
                    ok_g, graphed, err_g = run_section(graph, device)
                    if ok_g:
                        result["int8_sim_hipgraph_images_per_s"] = fwd_rate(graphed, 8)
                    elif err_g:
                        result["int8_sim_hipgraph_error"] = err_g
                    del graphed

                    def dual_graph():              # the same batch as two graphs of FB / 2 images on two streams
                        g2 = resident.capture(int8_net, batches[0], streams=2)
                        with torch.no_grad():
                            if not torch.equal(g2(batches[0]), res[0]):
                                raise RuntimeError("two-stream graph replay differs from the eager forward")
                        return g2
                    ok_d, dual, err_d = run_section(dual_graph, device) if FB % 2 == 0 else (False, None, None)
                    if ok_d:
                        result["int8_sim_dual_graph_images_per_s"] = fwd_rate(dual, 8)
                    elif err_d:
                        result["int8_sim_dual_graph_error"] = err_d
                    del dual
                else:
                    result["int8_sim_images_per_s"] = result.get("int8_sim_fp32_boundary_images_per_s")
                    if err_r:
                        result["int8_sim_resident_error"] = err_r
            for e in (err_t, err_i):
                if e:
                    result.setdefault("recon_errors", []).append(e)
        else:
            result["recon_error"] = err or "weight_quantize failed on another rank"

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline(lambda: build_model(args.model, HW, torch.device("cpu")), HW, images, q, log)
        except Exception as e:
            result["cpu_baseline"] = {"error": repr(e)}

    # ---- file inputs (reference pytorch_quantizer.py:252-284, PRE_PROCESS.IMG = 2: one .npy file per
    # calibration item): the SAME images as the timed region, written as .npy files outside the clock, calibrated through
    # the drop-in's file mode (Quantity.file_batch files per forward, decoded by a thread pool into pinned staging, H2D on a
    # side stream).  Never the headline: reported beside it with its ratio to the tensor-input rate.
    if world == 1 and args.input_mode in ("npy", "both") and not args.no_file_input and images > 16384:
        result["file_input"] = {"skipped": "%d images as one .npy file each is %.0f GB of scratch files; measured at the 5 120-image "
                                           "configuration" % (images, images * 3 * HW * HW * 4 / 1e9)}
    elif world == 1 and args.input_mode in ("npy", "both") and not args.no_file_input:
        try:
            import shutil
            import yaml
            fdir = tempfile.mkdtemp(prefix="fq_bench_npy_", dir=os.environ.get("FQ_BENCH_FILE_DIR") or None)
            paths = []
            t_w = time.perf_counter()
            for bi, xb in enumerate(data.owned()):
                host = xb.cpu().numpy()
                for j in range(host.shape[0]):
                    paths.append(os.path.join(fdir, "img_%05d.npy" % (bi * B + j)))
                    np.save(paths[-1], host[j])
            write_s = time.perf_counter() - t_w
            wd = make_workdir(len(paths) - 1, shape, dev_index)
            ucfg_path = os.path.join(wd, "test", "user_configs.yml")
            with open(ucfg_path) as fh:
                ucfg = yaml.safe_load(fh)
            ucfg["PRE_PROCESS"]["IMG"] = 2
            with open(ucfg_path, "w") as fh:
                yaml.safe_dump(ucfg, fh)
            # two runs, as for `value` (whose clock starts in a process that has calibrated before): the first one page-locks
            # its staging ring (6 x 154 MB, 10-20 ms each) inside its clock and is reported as first_run_images_per_s
            first_dt = None
            for _rep in range(2):
                fq = Quantity(model)
                fq.file_batch = B
                fq.profile_phases = True
                barrier()
                t0 = time.perf_counter()
                fq.activation_quantize(paths)
                barrier()
                dt = time.perf_counter() - t0
                if first_dt is None:
                    first_dt = dt
            same = open("./workdir/feat.table").read() == feat_table
            result["file_input"] = {"mode": "npy (PRE_PROCESS.IMG = 2)", "files": len(paths), "file_bytes": int(os.path.getsize(paths[0])),
                                    "files_per_forward": B, "decode_threads": fq.decode_workers, "seconds": round(dt, 3),
                                    "images_per_s": round(len(paths) / dt, 1), "ratio_to_tensor_inputs": round(len(paths) / dt / value, 3),
                                    "first_run_images_per_s": round(len(paths) / first_dt, 1),
                                    "same_table_as_tensor_inputs": bool(same), "write_files_s_outside_clock": round(write_s, 2),
                                    "pass1_s": round(fq.timings.get("pass1_s", 0.0), 4), "pass2_s": round(fq.timings.get("pass2_s", 0.0), 4),
                                    "host_wait_s": {k: round(v, 4) for k, v in getattr(fq, "input_wait_s", {}).items()}}
            del fq
            shutil.rmtree(fdir, ignore_errors=True)
        except Exception as e:
            result["file_input"] = {"error": repr(e)}

    # ---- per-channel rows (extension; BASELINE configs[1] words the workload "per-channel"): same two passes with
    # one histogram row per (tensor, channel), read in place by fq_absmax_chan / fq_hist2048_chan, then the KL sweep of
    # all 42 667 rows -- on the WHOLE workload (config 2's 5 120 images; up to round 5: 1 024 of them, where the sweep's fixed 47 ms
    # was a third of the time); strong-scaling jobs keep to 20 batches
    if world == 1 and not args.no_per_channel:
        try:
            n_pc = max(1, min(K, 20))
            pc_data = [(b, 0) for b in data.owned()[:n_pc]]
            make_workdir(len(pc_data) - 1, shape, dev_index)
            pq = Quantity(model)
            with CallTimer(_native, "hist2048_chan", _seg_bytes) as kt_pc:
                kt_pc.enabled = True
                barrier()
                t0 = time.perf_counter()
                pq.activation_quantize_per_channel(pc_data)
                barrier()
                dt = time.perf_counter() - t0
            result["per_channel_calibration"] = {"images": len(pc_data) * B, "rows": int(pq._channel_collector.rows),
                                                 "seconds": round(dt, 3), "images_per_s": round(len(pc_data) * B / dt, 1),
                                                 "kl_sweep_s": getattr(pq._channel_collector, "kl_seconds", None)}
            s = kt_pc.summary()
            if s:
                result["roofline_per_channel"] = hbm_roofline("hist2048_chan_kernel", s)
            del pq
        except Exception as e:
            result["per_channel_calibration"] = {"error": repr(e)}

    return finish()


if __name__ == "__main__":
    sys.exit(main() or 0)
