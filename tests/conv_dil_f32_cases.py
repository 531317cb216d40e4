"""The shapes the GPU tests of fq_conv_dil_f32 run and scripts/conv_dil_f32_geom_check.cpp walks: (N, Cin, Cout, H, W, d, pad)."""
SHAPES = [
    (1, 16, 4, 5, 5, 2, 2),            # one chunk pair, Cout = 4
    (2, 32, 20, 9, 11, 2, 2),          # four chunks, odd plane, Cout no tile multiple, batch 2
    (2, 16, 8, 7, 7, 6, 6),            # d about the size of the plane
    (1, 16, 8, 6, 6, 12, 12),          # only the centre tap live
    (1, 16, 8, 14, 14, 12, 12),        # taps live for part of a tile; two row bands
    (2, 16, 8, 9, 9, 3, 0),            # no padding, odd d
    (1, 16, 8, 8, 8, 2, 4),            # pad = 2d: the output is larger than the input
    (1, 16, 4, 3, 300, 2, 2),          # a row wider than one column block
    (16, 16, 8, 64, 64, 2, 2),         # more tiles than workgroups of the histogram grid: workgroups walk
    (16, 16, 72, 40, 40, 3, 3),        # 64-channel tiles (MT = 2), the second one partly filled
    (1, 16, 4, 20, 130, 33, 33),       # the staging limit lowers the band to 3 rows: three disjoint column runs of 32
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
