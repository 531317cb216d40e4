"""The launches of the atrous depthwise kernel that tests/test_gpu_atrous_depthwise_i8.py runs against the oracle and that
tests/test_atrous_plan_cpu.py hands to the host walker (scripts/dwconv_dil_geom_check.cpp): one list, so the walker walks what
the GPU runs.  (R, d, pad_h, pad_w, C, H, W, N, rs, relu); every plane is at most 40 pixels a side.

A lane's tile is TP x 4 outputs of one phase (TP = 4 for 3x3, 2 for 5x5).  What the list holds beyond the plain grid of
R x d x padding {0, d*(R//2), d*(R-1)}: H != W with W mod d != 0 (phases with unequal column counts: 9x13 at d = 4), phases with
fewer than four columns and fewer than TP rows (every d = 12 case, 12x17 at d = 4), planes smaller than d that exist only behind
their padding, so that only some taps ever land inside (5x7 at d = 6, 3x5 at d = 12), pad_h != pad_w, the ASPP extreme 14x14 at
d = 12, 33x29 at d = 2 (several bands and blocks per phase), and the same plane with 131 images of 100 channels: 18864 tiles of
28 lanes, more than the 2048 workgroups hold, so that lanes advance to a second tile (the carries of dwd_advance)."""

KERNEL_CASES = [
    (3, 2, 0, 0, 16, 9, 13, 1, 7, False), (3, 2, 2, 2, 19, 33, 29, 3, 1, True), (3, 2, 4, 4, 100, 7, 10, 1, 16, False),
    (3, 3, 0, 0, 1, 11, 14, 3, 7, True), (3, 3, 3, 3, 100, 10, 11, 1, 1, False), (3, 3, 6, 6, 16, 5, 7, 3, 16, True),
    (3, 4, 4, 4, 19, 9, 13, 3, 7, False), (3, 4, 0, 0, 16, 12, 17, 1, 1, True), (3, 4, 8, 8, 1, 6, 9, 1, 16, False),
    (3, 6, 6, 6, 100, 5, 7, 1, 7, True), (3, 6, 12, 12, 19, 14, 15, 1, 1, False), (3, 6, 0, 0, 16, 16, 19, 3, 16, True),
    (3, 12, 12, 12, 19, 14, 14, 1, 7, True), (3, 12, 24, 24, 16, 3, 5, 3, 1, False), (3, 12, 0, 0, 100, 27, 40, 1, 16, True),
    (5, 2, 0, 0, 19, 11, 14, 1, 7, True), (5, 2, 4, 4, 100, 9, 13, 3, 1, False), (5, 2, 8, 8, 16, 6, 9, 1, 16, True),
    (5, 3, 6, 6, 1, 13, 17, 3, 7, False), (5, 3, 12, 12, 19, 4, 5, 1, 1, True), (5, 4, 8, 8, 16, 9, 13, 1, 16, False),
    (5, 4, 0, 0, 100, 19, 22, 1, 7, True), (5, 6, 12, 12, 19, 15, 20, 1, 1, False), (5, 6, 24, 24, 16, 5, 7, 3, 7, True),
    (5, 12, 24, 24, 16, 14, 14, 1, 16, False), (3, 4, 4, 8, 19, 10, 15, 3, 7, True), (5, 2, 4, 4, 100, 33, 29, 131, 7, True),
]


def case_id(c):
    return "r%d_d%d_p%dx%d_c%d_%dx%d_n%d_rs%d_relu%d" % c


def walker_arg(c):
    R, d, ph, pw, C, H, W, N = c[:8]
    return "%d,%d,%d,%d,%d,%d,%d,%d" % (R, d, N, H, W, C, ph, pw)
