#!/usr/bin/env python3
"""Compare the dense int8 convolution launches of two builds from their rocprofv3 kernel traces.

    for s in default "halo8=2" ...:      (the settings of tests/conv_select_cases.py, one process each)
        rocprofv3 --kernel-trace --output-format csv -d A/$i -- python scripts/ab_lib.py A.so scripts/int8_conv_choice_dump.py --setting "$s"
        rocprofv3 --kernel-trace --output-format csv -d B/$i -- python scripts/int8_conv_choice_dump.py --setting "$s"
    python scripts/conv_select_trace_diff.py A B

Needs no GPU.  Under A and B every sub-directory is one setting; its *kernel_trace.csv rows whose kernel is one of fq_conv_i8.hip's
are taken in dispatch order as (kernel name with its template arguments, grid, workgroup, LDS bytes) and must be equal, row for
row: the variant code says which kernel family ran, this says which instantiation, on which grid, with how much LDS.  Prints one
line per setting and the distinct instantiations seen; exit status 1 on a difference."""
import csv
import glob
import os
import sys

KERNELS = ("conv2d_i8_kernel", "conv2d_i8_dma_kernel", "conv3x3_i8_halo_kernel", "conv3x3_i8_halo8_kernel", "conv3x3_i8_c64_kernel",
           "linear_i8_wave_kernel")


def _get(row, *names):
    for n in names:
        if n in row:
            return row[n]
    return "?"


def launches(folder):
    rows = []
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                if any(k in name for k in KERNELS):
                    grid = "x".join(_get(r, "Grid_Size_" + a, "Grid_Size") for a in "XYZ")
                    wg = "x".join(_get(r, "Workgroup_Size_" + a, "Workgroup_Size") for a in "XYZ")
                    rows.append((int(_get(r, "Dispatch_Id", "Start_Timestamp")), name.split("(")[0], grid, wg,
                                 _get(r, "LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v")))
    return [r[1:] for r in sorted(rows)]


def main(a, b):
    bad = 0
    seen = set()
    subs = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    for s in subs:
        ra, rb = launches(os.path.join(a, s)), launches(os.path.join(b, s))
        same = ra == rb and len(ra) > 0
        bad += not same
        seen.update(ra)
        print("%-8s %4d launches in %s, %4d in %s: %s" % (s, len(ra), a, len(rb), b, "equal, row for row" if same else "DIFFERENT"))
        if not same:
            for i, (x, y) in enumerate(zip(ra, rb)):
                if x != y:
                    print("   first difference at launch %d:\n     %s\n     %s" % (i, x, y))
                    break
    print("%d distinct (kernel instantiation, grid, workgroup, LDS) rows:" % len(seen))
    for row in sorted(seen):
        print("   %s  grid %s  workgroup %s  lds %s" % row)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
