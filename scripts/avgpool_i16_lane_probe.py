"""Lane ownership of the average pool over an int16 sum: the library's 8 channels per lane
(fq_avgpool_i16_nhwc) against the 16-channel form of scripts/avgpool_i16_c16_probe.hip at the three shortcut shapes of ResNet-50-D,
256 images, 2x2 / 2.  The probe's output is compared with the library's first (also on an odd plane with masked channels), then
five alternating rounds of 200 back-to-back launches are timed between device events; medians, minima and maxima are printed
(-> profiles/r19_avgpool_sum.txt).  Build the probe library first (the command is in the .hip file's header); scripts/_bin/ is
git-ignored.

    python scripts/avgpool_i16_lane_probe.py
"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT]
from common.quantity import _native
v = ctypes.CDLL(os.path.join(ROOT, "scripts", "_bin", "libavg16c.so"))
v.avg16c_launch.restype = ctypes.c_int
v.avg16c_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 14 + [ctypes.c_void_p]
N = 256
def c16(q, out, C):
    n, H, W, cpad = q.shape
    rc = v.avg16c_launch(q.data_ptr(), out.data_ptr(), n, H, W, C, cpad, 2, 2, 2, 2, 0, 0, 1, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
def c8(q, out, C):
    _native.avgpool_i16_nhwc(q, C, (2, 2), (2, 2), (0, 0), True, 0, False, out=out)
def timed(fn, q, out, C, iters=200):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn(q, out, C)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3
for (hw, C) in ((56, 256), (28, 512), (14, 1024)):
    q = torch.randint(-32768, 32768, (N, hw, hw, C), dtype=torch.int16, device="cuda")
    a = torch.empty(N, hw // 2, hw // 2, C, dtype=torch.int8, device="cuda"); b = torch.zeros_like(a)
    c8(q, a, C); c16(q, b, C); torch.cuda.synchronize()
    assert torch.equal(a, b), "the two forms disagree"
    # a small odd case with masked channels too
    qs = torch.randint(-32768, 32768, (3, 5, 7, 32), dtype=torch.int16, device="cuda")
    sa = torch.empty(3, 2, 3, 32, dtype=torch.int8, device="cuda"); sb = torch.zeros_like(sa)
    c8(qs, sa, 19); c16(qs, sb, 19); torch.cuda.synchronize()
    assert torch.equal(sa, sb)
    nbytes = N * C * (2 * hw * hw + (hw // 2) ** 2)
    r8, r16 = [], []
    for r in range(5):
        r8.append(timed(c8, q, a, C)); r16.append(timed(c16, q, b, C))
    m8, m16 = float(np.median(r8)), float(np.median(r16))
    print("%3dx%-3d x %4d channels, %7.2f MB: 8 per lane %6.1f us (%4.0f GB/s; min %.1f max %.1f), 16 per lane %6.1f us (%4.0f GB/s; min %.1f max %.1f)"
          % (hw, hw, C, nbytes / 1e6, m8, nbytes / m8 / 1e3, min(r8), max(r8), m16, nbytes / m16 / 1e3, min(r16), max(r16)), flush=True)
