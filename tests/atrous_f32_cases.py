"""Shared by tests/test_gpu_atrous_depthwise_f32.py, tests/test_atrous_f32_cpu.py and scripts/dwconv_dil_f32_geom_check.cpp (test
infrastructure, no product code): the launch shapes of the atrous depthwise float convolution fq_dwconv_dil_f32."""

# N, C, H, W, R, d, pad: odd, unaligned rows; the ASPP rates on a 14 x 14 plane (at d = 18 only the centre tap is in the image);
# 5x5; no padding (the output shrinks); pad < d; pad equal to the span; several bands per plane; more planes than one tile holds;
# the largest d.  Then what csrc/fq_dwconv_dil_f32_geom.h adds: a plane taller than one tile's LDS (row bands of TH >= d rows,
# one merged run of staged rows), and a wide one at a large d (row bands of TH < d rows, R disjoint runs; two column blocks)
SHAPES = [(2, 3, 5, 7, 3, 2, 2), (1, 5, 14, 14, 3, 6, 6), (2, 4, 14, 14, 3, 12, 12), (2, 4, 14, 14, 3, 18, 18), (1, 2, 9, 11, 5, 2, 4),
          (1, 2, 20, 9, 3, 3, 0), (1, 3, 12, 10, 3, 4, 1), (1, 2, 6, 6, 3, 2, 4), (1, 2, 70, 33, 3, 2, 2), (3, 130, 7, 7, 3, 2, 2),
          (1, 1, 3, 5, 3, 64, 64), (1, 1, 200, 33, 3, 2, 2), (1, 1, 40, 300, 3, 20, 20)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
