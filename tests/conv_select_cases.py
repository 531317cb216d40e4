"""The layers whose kernel choice is held: by scripts/conv_i8_select_check.cpp on the host (tests/test_conv_i8_select_cpu.py) and, one
launch each, by scripts/int8_conv_choice_dump.py on the GPU (tests/golden/g21_int8_conv_choice.txt is its record of the tree before
the selector existed).  A case is the checker's argument: N,H,W,C,K,R,S,sh,sw,ph,pw,dh,dw/outs[/pcs] with C already padded to 16;
outs is y, q, yq or add."""

CUS = 256            # csrc/fq_common.h: kCUs


def case(N, C, H, W, K, R, S=None, stride=1, pad=0, outs="q", pcs=False, dil=1):
    S = R if S is None else S
    cpad = (C + 15) // 16 * 16
    return "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d/%s%s" % (N, H, W, cpad, K, R, S, stride, stride, pad, pad, dil, dil, outs,
                                                             "/pcs" if pcs else "")


# ---- what today only a GPU asserts (copies: the GPU tests keep theirs) -----------------------------------------------------
# tests/test_gpu_resident.py: RES_CASES (N, C, H, W, K, R, S, stride, pad, kernel), each in the three output forms that test runs
RES_CASES = [
    (2, 16, 8, 8, 64, 3, 3, 1, 1, "tile_general/64"),
    (3, 32, 9, 7, 40, 3, 3, 2, 1, "tile_general/64"),
    (2, 128, 7, 7, 200, 3, 3, 1, 1, "tile_general/64"),
    (1, 256, 6, 6, 512, 1, 1, 2, 0, "tile_c128/64"),
    (40, 128, 14, 14, 256, 1, 1, 1, 0, "tile_c128/64"),
    (2, 3, 20, 20, 10, 3, 3, 1, 1, "tile_general/64"),
]
RES_EXPECT = [(case(N, C, H, W, K, R, S, st, pd, outs), want) for (N, C, H, W, K, R, S, st, pd, want) in RES_CASES
              for outs in ("q", "yq", "y")]
# tests/test_gpu_conv_i8.py: test_linear_i8_vs_oracle's (N, F, K), and the 1 x 1 planes of the bias test (linear_wave; with pad 1 and
# stride 3 NOT linear_wave)
LINEAR_SHAPES = ((4, 512, 10), (64, 2048, 1000), (3, 400, 120), (1, 84, 10), (300, 272, 37), (256, 2048, 1000))
LINEAR_EXPECT = [(case(N, F, 1, 1, K, 1, outs="y"), "linear_wave/32") for N, F, K in LINEAR_SHAPES] + \
    [(case(37, 64, 1, 1, 128, 1, outs="y"), "linear_wave/32")]
NOT_LINEAR = case(37, 64, 1, 1, 128, 1, stride=3, pad=1, outs="y")
# tests/test_gpu_r50_tables.py: the 3x3 layers of ResNet-50 (C = K, plane of the INPUT, stride, how many there are).  At 256 images:
# three on c64_halo/64, at least 7 on halo8, all 13 stride-1 ones on the halo kernels, the three stride-2 ones on LDS-DMA; at 2
# images no halo8.
R50_3X3 = ((64, 56, 1, 3), (128, 56, 2, 1), (128, 28, 1, 3), (256, 28, 2, 1), (256, 14, 1, 5), (512, 14, 2, 1), (512, 7, 1, 2))


def r50_3x3(batch):
    return [(case(batch, c, hw, hw, c, 3, stride=st, pad=1), st, count) for c, hw, st, count in R50_3X3]


# ---- the three chip-filling thresholds, each at kCUs - 1, kCUs, kCUs + 1 workgroups (C = K = 128) -----------------------------
AROUND = (CUS - 1, CUS, CUS + 1)
# wg128 = ceil(M / 128) * ceil(K / 128) < kCUs: 64-row tiles.  One image of g x 128 pixels: g pixel tiles
TK_1X1 = [case(1, 128, g, 128, 128, 1) for g in AROUND]
TK_3X3 = [case(1, 128, 4 * g, 32, 128, 3, pad=1) for g in AROUND]
# grid.x * grid.y <= kCUs: the LDS-DMA kernel's ring of 3.  3x3 / stride 2 / pad 1 (no halo form) on 2g x 256 pixels: g pixel
# tiles.  By default g < kCUs runs 64-row tiles, 2g workgroups -- so also g = kCUs / 2 and one more; under FQ_CONV_TK=128 the three
# around kCUs are g workgroups each
RING_3X3 = [case(1, 128, 2 * g, 256, 128, 3, stride=2, pad=1) for g in AROUND + (CUS // 2, CUS // 2 + 1)]
# ceil(M / 256) * (K / TK) >= kCUs: the eight-wave halo kernel.  8g x 32 pixels: g tiles of 256 (the largest case of the list)
HALO8_3X3 = [case(1, 128, 8 * g, 32, 128, 3, pad=1) for g in AROUND]
# rows too wide for a slab of 130 + 2 W pixels in half a CU's LDS: W = 128 still fits (ring of 3 at TK 64), W = 256 does not -> LDS-DMA
WIDE_3X3 = [case(1, 128, 32, 128, 128, 3, pad=1), case(1, 128, 16, 256, 128, 3, pad=1)]

# ---- small layers for the switch settings -----------------------------------------------------------------------------------
HALO_SMALL = [case(2, 256, 14, 14, 256, 3, pad=1), case(2, 256, 14, 14, 256, 3, pad=1, outs="yq"),
              case(2, 128, 9, 7, 128, 3, pad=1, outs="y", pcs=True), case(3, 128, 5, 5, 64, 3, pad=1, pcs=True),
              case(2, 64, 12, 12, 64, 3, pad=1), case(2, 64, 12, 12, 48, 3, pad=1, outs="yq", pcs=True)]
DEEP_SMALL = [case(2, 128, 14, 14, 128, 3, stride=2, pad=1), case(2, 1024, 7, 7, 256, 1), case(2, 1024, 7, 7, 256, 1, outs="add"),
              case(2, 1024, 7, 7, 256, 1, outs="add", pcs=True), case(2, 128, 9, 9, 128, 3, pad=2, dil=2, outs="yq")]
SHALLOW_SMALL = [case(2, 256, 7, 7, 1024, 1, outs="add"), case(2, 64, 9, 9, 256, 1), case(2, 64, 9, 9, 256, 1, outs="add", pcs=True),
                 case(2, 48, 9, 9, 100, 1, outs="yq"), case(2, 64, 9, 9, 128, 1, outs="y")]

# ---- the settings: (name, switches as NAME=value, cases).  "default" holds every expectation above that a launch can record --------
SETTINGS = [
    ("default", (), [c for c, _ in RES_EXPECT + LINEAR_EXPECT] + [NOT_LINEAR] + [c for c, _, _ in r50_3x3(2)] + TK_1X1 + TK_3X3 +
     RING_3X3 + HALO8_3X3 + WIDE_3X3 + HALO_SMALL + DEEP_SMALL + SHALLOW_SMALL),
    ("halo8=2", ("FQ_HALO8=2",), HALO_SMALL),
    ("halo8=2 halo_stages=3", ("FQ_HALO8=2", "FQ_HALO_STAGES=3"), HALO_SMALL),
    ("halo_np=2", ("FQ_HALO_NP=2",), HALO_SMALL[:4]),
    ("tk=128", ("FQ_CONV_TK=128",), RING_3X3[:3] + DEEP_SMALL + SHALLOW_SMALL + HALO_SMALL[:2]),
    ("tk=128 stages=2", ("FQ_CONV_TK=128", "FQ_CONV_STAGES=2"), RING_3X3[:3] + DEEP_SMALL),
    ("dma=0", ("FQ_CONV_DMA=0",), HALO_SMALL[:4] + DEEP_SMALL),
]
