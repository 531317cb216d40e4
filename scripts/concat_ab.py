"""Time the int8 concat entry points of two builds of libfq_hip.so against each other on one GPU.

    python scripts/concat_ab.py OLD.so NEW.so [--rounds 7] [--out FILE]

One process loads both libraries with ctypes and calls fq_concat_i8_nhwc / fq_concat_n_i8_nhwc directly (the C ABI is the same in
both, so one argument block serves both).  Per shape: the outputs of the two libraries are compared for equality, every arm is
warmed up, then `rounds` rounds of old, new, old again, each timed with device events around enough launches that a round lasts
about 30 ms; the launches rotate over several buffer sets so that the working set is larger than the last-level cache.  Prints
median / min / max / spread per arm, algorithmic bytes (sources read + output written) and TB/s from the median, and the rule:
new median <= old median + the old arm's spread (max - min over its rounds).  Exit status 1 when a shape misses the rule or an
output differs.  Shapes are workload shapes at 256 images."""
import argparse
import ctypes
import statistics
import sys

import torch


class CatSrc(ctypes.Structure):
    _fields_ = [("q", ctypes.c_void_p), ("C", ctypes.c_int), ("Cpad", ctypes.c_int), ("up", ctypes.c_int)]


class CatSrcN(ctypes.Structure):
    _fields_ = [("q", ctypes.c_void_p), ("C", ctypes.c_int), ("Cpad", ctypes.c_int), ("up", ctypes.c_int), ("relu", ctypes.c_int)]


# (name, entry, N, H, W, channels, factors)
SHAPES = [
    ("inception [96,128] 14x14, two-source aligned", "two", 256, 14, 14, [96, 128], [1, 1]),
    ("fire [64,64] 55x55, two-source aligned", "two", 256, 55, 55, [64, 64], [1, 1]),
    ("[20,44] 56x56, two-source general", "two", 256, 56, 56, [20, 44], [1, 1]),
    ("fpn [256,256] 28x28 up (1,2), two-source upsampled", "two", 256, 28, 28, [256, 256], [1, 2]),
    ("[32,48,32,16] 28x28, eight-entry aligned", "n", 256, 28, 28, [32, 48, 32, 16], [1, 1, 1, 1]),
    ("[20,44,13] 56x56, eight-entry general", "n", 256, 56, 56, [20, 44, 13], [1, 1, 1]),
]


def pad16(c):
    return (c + 15) // 16 * 16


def load(path):
    L = ctypes.CDLL(path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    L.fq_concat_i8_nhwc.restype = ci
    L.fq_concat_i8_nhwc.argtypes = [ctypes.POINTER(CatSrc), ci, vp, ci, ci, ci, ci, ci, vp]
    L.fq_concat_n_i8_nhwc.restype = ci
    L.fq_concat_n_i8_nhwc.argtypes = [ctypes.POINTER(CatSrcN), ci, vp, ci, ci, ci, ci, vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    libs = {"old": load(a.old), "new": load(a.new)}
    lines, failed = [], False

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("concat entry points, old = %s, new = %s, %s, %d rounds of old / new / old again" % (a.old, a.new, torch.cuda.get_device_name(0), a.rounds))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, entry, N, H, W, Cs, ups in SHAPES:
        cpad_out = pad16(sum(Cs))
        nbytes = sum(N * (H // u) * (W // u) * pad16(c) for c, u in zip(Cs, ups)) + N * H * W * cpad_out
        nset = max(2, min(16, -(-600_000_000 // nbytes)))
        sets = []
        for _ in range(nset):
            srcs = [torch.randint(-128, 128, (N, H // u, W // u, pad16(c)), dtype=torch.int8, device="cuda", generator=gen) for c, u in zip(Cs, ups)]
            out = torch.empty(N, H, W, cpad_out, dtype=torch.int8, device="cuda")
            if entry == "two":
                arr = (CatSrc * len(Cs))(*[CatSrc(s.data_ptr(), c, pad16(c), u) for s, c, u in zip(srcs, Cs, ups)])
            else:
                arr = (CatSrcN * len(Cs))(*[CatSrcN(s.data_ptr(), c, pad16(c), u, 1) for s, c, u in zip(srcs, Cs, ups)])
            sets.append((srcs, out, arr))

        def launch(L, k):
            _s, out, arr = sets[k % nset]
            if entry == "two":
                rc = L.fq_concat_i8_nhwc(arr, len(Cs), out.data_ptr(), cpad_out, 1, N, H, W, None)
            else:
                rc = L.fq_concat_n_i8_nhwc(arr, len(Cs), out.data_ptr(), cpad_out, N, H, W, None)
            assert rc == 0, (name, rc)

        # equality of the two builds at the timed size
        got = {}
        for arm, L in libs.items():
            sets[0][1].fill_(77)
            launch(L, 0)
            torch.cuda.synchronize()
            got[arm] = sets[0][1].clone()
        equal = torch.equal(got["old"], got["new"]) and bool((got["new"][..., sum(Cs):] == 0).all()) and int(got["new"].max()) > 0
        del got

        def timed(L, count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(count):
                launch(L, k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / count                   # microseconds per launch

        for L in libs.values():
            timed(L, 4 * nset)
        count = max(50, min(5000, int(30000.0 / max(timed(libs["old"], 4 * nset), 1.0))))
        t = {"old": [], "new": [], "old again": []}
        for _ in range(a.rounds):
            t["old"].append(timed(libs["old"], count))
            t["new"].append(timed(libs["new"], count))
            t["old again"].append(timed(libs["old"], count))
        say("%s: %.2f MB per launch, %d buffer sets, %d launches per round, outputs %s" % (name, nbytes / 1e6, nset, count, "equal" if equal else "DIFFER"))
        for arm in ("old", "new", "old again"):
            v = t[arm]
            med = statistics.median(v)
            say("    %-9s median %8.2f us  min %8.2f  max %8.2f  spread %6.2f  %.2f TB/s" % (arm, med, min(v), max(v), max(v) - min(v), nbytes / med / 1e6))
        old_med, new_med, spread = statistics.median(t["old"]), statistics.median(t["new"]), max(t["old"]) - min(t["old"])
        ok = new_med <= old_med + spread
        say("    new - old = %+.2f us (%+.2f %%), old arm's spread %.2f us: %s" % (new_med - old_med, 100 * (new_med - old_med) / old_med, spread, "within the rule" if ok else "MISSES the rule"))
        failed = failed or not ok or not equal
        del sets
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
