// fq_conv_i8_select.h -- which kernel a dense int8 convolution runs on (fq_conv_i8.hip), and with which tile height, ring depth,
// grid, workgroup order and dynamic LDS: the environment switches, parsed once, and ONE pure function from (geometry, wanted
// outputs, switches) to a ConvChoice.  Plain host C++ without a HIP include, kept apart from the kernels so that the same
// function compiles into scripts/conv_i8_select_check.cpp, which prints the choice of any layer and asserts its invariants on
// a box without a GPU (tests/test_conv_i8_select_cpu.py).
//
// The order of the families (DESIGN.md section 25 has it as one table):
//   1. c64_halo       3x3 / stride 1 / pad 1, C == 64, K <= 64, no fused add: stationary weights, persistent workgroups
//   (2. the streaming 1x1 kernel, fq_conv1x1_i8.hip: its own switches and its own predicate; the dispatcher asks it unless the
//       choice here is c64_halo.  It is not part of this function.)
//   3. linear_wave    a 1x1 plane, pad 0, dilation 1, an fp32 output alone
//   4. the tiles      TK = 64 when the output is narrow or 128-row tiles would not give one workgroup per CU; then, for
//                     C % 128 == 0 and K % TK == 0 and a deep reduction: halo8, halo, dma2 / dma3; for C % 128 == 0 and
//                     K % TK == 0: tile_c128; for C == 64: tile_c64; else tile_general
// A family whose kernel needs the dynamic-LDS attribute can be refused by the runtime at launch; the dispatcher then asks again
// with that family in `excluded` (c64_halo: whatever is next; halo8 AND halo are one family here: a refused halo8 falls to the
// LDS-DMA kernel, not to the 128-pixel halo).
//
// Everything lives in fq::sel with its own copies of the few constants it shares with the kernels; fq_conv_i8.hip holds them
// equal with static_asserts.  The functions are static: the library exports none of them.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace fq {
namespace sel {

constexpr int kCUs = 256;                // MI355X
constexpr int kTP = 128;                 // pixels per workgroup tile
constexpr int kConvBlock = 256;
constexpr int kLinWaves = 4;             // waves of a linear_wave workgroup
// fq_conv2d_i8_last_variant (fq_common.h: ConvVariant)
constexpr int kVarC64Halo = 1, kVarHalo8 = 3, kVarHalo = 4, kVarDma2 = 5, kVarDma3 = 6, kVarTileC128 = 7, kVarTileC64 = 8,
              kVarTileGeneral = 9, kVarLinearWave = 13;
// kOut bits and kPath of the kernel templates (fq_conv_i8_common.h, fq_conv_i8.hip)
constexpr int kOutF32 = 1, kOutI8 = 2, kOutAdd = 4, kOutPcs = 16;
constexpr int kPathGeneral = 0, kPathC128 = 1, kPathC64 = 2;
// Families: which kernel template a choice launches, and the bits of `excluded`.
constexpr unsigned kFamC64Halo = 1, kFamHalo = 2, kFamDma = 4, kFamTile = 8, kFamLinear = 16;

// ---- the switches ----------------------------------------------------------------------------------------------------------
// One field per environment variable of the dense int8 dispatch, each with the parse rule it has always had:
//   on/off   on unless the value starts with '0' (unset and "" are on)
//   number   atoi of the value, a default when unset ("" is 0)
//   FQ_CONV_DMA   unset: by the depth of the reduction; a value starting with '0': off; anything else, "" included: on
struct ConvSwitches {
    bool xcd;              // FQ_CONV_XCD        on/off   0: plain 2-D grid (A/B timing)
    int stages;            // FQ_CONV_STAGES     number, 0   ring depth of the LDS-DMA kernel (0: by the size of the launch)
    bool halo;             // FQ_CONV_HALO       on/off   the halo form of the 3x3 layers
    int halo_stages;       // FQ_HALO_STAGES     number, 0   its weight ring (0: 2 for halo8, what fits for halo)
    int halo_np;           // FQ_HALO_NP         number, 0   2: 256-pixel tiles on four waves (slower; never halo8)
    int halo8;             // FQ_HALO8           number, 1   0: never, 1: chip-filling launches, 2: everywhere
    bool c64_halo;         // FQ_CONV_C64_HALO   on/off
    bool c64_xcd;          // FQ_C64_XCD         on/off   0: the c64 kernel deals its tiles round robin
    int c64_wg_per_cu;     // FQ_C64_WG_PER_CU   number, 2   persistent workgroups per CU
    bool linear_wave;      // FQ_LINEAR_WAVE     on/off
    int dma;               // FQ_CONV_DMA        -1 / 0 / 1 (above)
    int tk;                // FQ_CONV_TK         number, 0   64 / 128 force the tile height
    bool c64;              // FQ_CONV_C64        on/off   the C == 64 path of the register-staged kernel
};

// get: getenv in the library (once per process), a getter over argv in the checker
static inline ConvSwitches read_conv_switches(const char* (*get)(const char*)) {
    const auto on = [&](const char* name) { const char* e = get(name); return !(e && e[0] == '0'); };
    const auto num = [&](const char* name, int unset) { const char* e = get(name); return e ? atoi(e) : unset; };
    ConvSwitches s;
    s.xcd = on("FQ_CONV_XCD");
    s.stages = num("FQ_CONV_STAGES", 0);
    s.halo = on("FQ_CONV_HALO");
    s.halo_stages = num("FQ_HALO_STAGES", 0);
    s.halo_np = num("FQ_HALO_NP", 0);
    s.halo8 = num("FQ_HALO8", 1);
    s.c64_halo = on("FQ_CONV_C64_HALO");
    s.c64_xcd = on("FQ_C64_XCD");
    s.c64_wg_per_cu = num("FQ_C64_WG_PER_CU", 2);
    s.linear_wave = on("FQ_LINEAR_WAVE");
    const char* d = get("FQ_CONV_DMA");
    s.dma = d ? (d[0] == '0' ? 0 : 1) : -1;
    s.tk = num("FQ_CONV_TK", 0);
    s.c64 = on("FQ_CONV_C64");
    return s;
}

// ---- the choice ------------------------------------------------------------------------------------------------------------
struct ConvOuts {
    bool y, q, res, pcs;   // fp32 NCHW output, int8 NHWC output, fused residual add, one shift per output channel
};

struct ConvChoice {
    int variant, tk;                     // what note_conv_variant records
    unsigned family;                     // kFam*: the kernel template; with it the template integers that template has
    int path, stages, np, out;           // kPath (tile), ring depth (dma, halo8, halo), sub-tiles per wave (halo), kOut bits
    unsigned grid_x, grid_y, block;
    unsigned lds;                        // dynamic LDS bytes (0: none, no attribute needed)
    int xcd_kt, tiles_m;                 // ConvParams: the XCD-aware workgroup order (conv_tile_of)
    int slab_rows, total_pixels;         // HaloParams / C64Params
    int tiles, xcd_chunk;                // C64Params
};

// Dynamic LDS a kernel of the halo family may ask for and still run two workgroups per CU (160 KB): half the CU's LDS minus what
// the kernel declares STATICALLY beside its dynamic carve-out -- sLH[2][TK] ints, the merged clamp bounds of the integer tail --
// and the allocation granule.  (The budget used to ignore the static part; no shape fell into the gap, but one layout change
// could have halved the occupancy silently.)
// (pcs: a kOutPcs kernel also declares sRs[TK], each channel's shift)
constexpr size_t two_per_cu_lds(int tk, bool pcs = false) { return (size_t)80 * 1024 - 64 - (size_t)(pcs ? 12 : 8) * tk; }

// The 2-D grid (gx pixel tiles, gy output-channel tiles) as the kernels are launched: 1-D, padded to 8 pixel tiles and decoded by
// conv_tile_of so that all channel tiles of a pixel tile run on one XCD -- unless there is one channel tile, the switch is off,
// or the padded grid would leave 31 bits.
static inline void xcd_grid(ConvChoice& c, unsigned gx, unsigned gy, const ConvSwitches& sw) {
    c.grid_x = gx; c.grid_y = gy;
    c.xcd_kt = 0;
    c.tiles_m = (int)gx;
    if (sw.xcd && gy > 1 && (long)((gx + 7) / 8) * 8 * gy < 0x7fffffffL) {
        c.xcd_kt = (int)gy;
        c.grid_x = ((gx + 7) / 8) * 8 * gy; c.grid_y = 1;
    }
}

// G: any struct with the geometry fields of ConvParams (N H W C K R S P Q, strides, pads, dilations, M, chunks).
template <class G>
static inline bool halo_shape(const G& p, const ConvOuts& o) {   // 3x3, stride 1, pad 1: a tap is a row offset into one slab of input pixels
    return p.R == 3 && p.S == 3 && p.stride_h == 1 && p.stride_w == 1 && p.pad_h == 1 && p.pad_w == 1 && p.dil_h == 1 &&
           p.dil_w == 1 && !o.res;
}

// the halo forms of a 3x3 layer with C % 128 == 0 and K % tk == 0; false: the LDS-DMA kernel takes it
template <class G>
static inline bool select_halo(ConvChoice& out, const G& p, const ConvOuts& o, const ConvSwitches& sw, int tk) {
    if (!sw.halo || !halo_shape(p, o)) return false;
    ConvChoice c = out;                  // (variant-independent fields are set; `out` changes only when a halo form is chosen)
    c.family = kFamHalo;
    c.total_pixels = p.N * p.H * p.W;
    const size_t budget = two_per_cu_lds(tk, o.pcs);
    // 256-pixel tiles on eight waves (conv3x3_i8_halo8_kernel) where that fills the chip: FQ_HALO8=0 keeps the 128-pixel form
    if (sw.halo8 && !sw.halo_np && (sw.halo8 > 1 || (((long)p.M + 255) / 256) * (p.K / tk) >= kCUs)) {
        c.slab_rows = (2 * 128 + 2 + 2 * p.W + 7) & ~7;
        c.stages = sw.halo_stages ? sw.halo_stages : 2;
        const size_t lds = (size_t)c.stages * tk * 128 + (size_t)tk * 8 + 128 + (size_t)c.slab_rows * 128;
        if (lds <= budget && (c.stages == 2 || c.stages == 3)) {
            c.variant = kVarHalo8;
            c.np = 1;
            c.block = 2 * kConvBlock;
            c.lds = (unsigned)lds;
            xcd_grid(c, (unsigned)(((long)p.M + 255) / 256), (unsigned)(p.K / tk), sw);
            out = c;
            return true;
        }
    }
    // 128-pixel tiles.  (FQ_HALO_NP=2: 256-pixel tiles, two sub-tiles per wave -- bit-exact, fewer LDS reads and barriers per
    // MFMA, and 20-35 % SLOWER on ResNet-50's layers at 256 images: 48.7 vs 39.9 us on 256 -> 256 @14x14.)
    c.np = sw.halo_np ? sw.halo_np : 1;
    c.slab_rows = (128 * c.np + 2 + 2 * p.W + 7) & ~7;
    const size_t fixed = (size_t)tk * 8 + 128 + (size_t)c.slab_rows * 128;
    c.stages = sw.halo_stages ? sw.halo_stages : ((size_t)3 * tk * 128 + fixed <= budget ? 3 : 2);
    const size_t lds = (size_t)c.stages * tk * 128 + fixed;
    if (lds > budget || (c.stages != 2 && c.stages != 3) || (c.np != 1 && c.np != 2)) return false;   // two workgroups per CU
    c.variant = kVarHalo;
    c.block = kConvBlock;
    c.lds = (unsigned)lds;
    xcd_grid(c, (unsigned)(((long)p.M + 128 * c.np - 1) / (128 * c.np)), (unsigned)(p.K / tk), sw);
    out = c;
    return true;
}

template <class G>
static inline ConvChoice select_conv_i8(const G& p, const ConvOuts& o, const ConvSwitches& sw, unsigned excluded = 0) {
    ConvChoice c = {};
    c.out = (o.res ? kOutI8 | kOutAdd : (o.y && o.q ? kOutF32 | kOutI8 : (o.q ? kOutI8 : kOutF32))) | (o.pcs ? kOutPcs : 0);
    // the 64 -> 64 3x3 layers: stationary weights, persistent workgroups
    if (!(excluded & kFamC64Halo) && sw.c64_halo && halo_shape(p, o) && p.C == 64 && p.K <= 64) {
        const int slab_rows = (130 + 2 * p.W + 15) & ~15;
        const size_t lds = (size_t)9 * 64 * 64 + 64 * 8 + 64 + (size_t)kTP * 80 + (size_t)2 * slab_rows * 64;
        if (lds <= two_per_cu_lds(64, o.pcs)) {              // two workgroups per CU
            c.variant = kVarC64Halo; c.tk = 64; c.family = kFamC64Halo;
            c.slab_rows = slab_rows;
            c.total_pixels = p.N * p.H * p.W;
            c.tiles = (int)(((long)p.M + kTP - 1) / kTP);
            c.xcd_chunk = sw.c64_xcd ? (c.tiles + 7) / 8 : 0;
            c.tiles_m = c.tiles;
            c.grid_x = (unsigned)(kCUs * sw.c64_wg_per_cu);
            if ((long)c.grid_x > c.tiles) c.grid_x = (unsigned)c.tiles;
            c.grid_y = 1; c.block = kConvBlock;
            c.lds = (unsigned)lds;
            return c;
        }
    }
    // a linear layer with an fp32 output: one workgroup per 32 x 32 tile, operands straight from L2 (FQ_LINEAR_WAVE=0: the tiles)
    // (pad 0, dilation 1: with padding and a stride >= 3 the one output pixel would sample the zero border, not x)
    if (sw.linear_wave && p.H == 1 && p.W == 1 && p.R == 1 && p.S == 1 && p.P == 1 && p.Q == 1 && p.pad_h == 0 && p.pad_w == 0 &&
        p.dil_h == 1 && p.dil_w == 1 && o.y && !o.q && !o.res && ((long)p.M + 31) / 32 <= 65535) {
        c.variant = kVarLinearWave; c.tk = 32; c.family = kFamLinear;
        c.grid_x = (unsigned)((p.K + 31) / 32); c.grid_y = (unsigned)(((long)p.M + 31) / 32); c.block = 64 * kLinWaves;
        return c;
    }
    const unsigned gx = (unsigned)(((long)p.M + kTP - 1) / kTP);
    // 64-row tiles when the output is narrow, or when 128-row tiles would not even give one workgroup per CU
    const long wg128 = (long)gx * ((p.K + 127) / 128);
    const int tk = ((p.K <= 64 || wg128 < kCUs || sw.tk == 64) && sw.tk != 128) ? 64 : 128;
    c.tk = tk;
    // Deep reductions (>= 8 K-steps: the 3x3 layers and the wide 1x1 reductions) are bound by L1/L2 request
    // throughput and run faster with coalesced LDS-DMA staging; shallow ones are output-bound, and there the
    // register-staged kernel's smaller LDS footprint (3 workgroups per CU instead of 2) wins.  Measured per
    // layer on ResNet-50 at batch 128 (scripts/conv_bench.py); FQ_CONV_DMA=0/1 forces one of them.
    const bool use_dma = sw.dma < 0 ? (p.chunks >> 3) >= 8 : sw.dma == 1;
    const bool whole = p.C % 128 == 0 && p.K % tk == 0;     // 128-byte K-steps, no partial channel tile
    c.block = kConvBlock;
    if (whole && use_dma) {
        if (!(excluded & kFamHalo) && select_halo(c, p, o, sw, tk)) return c;
        c.family = kFamDma;
        // A ring of 3 takes the DMA latency off the per-step critical path (one wave's step: 1 960 -> 1 700 cycles) but
        // needs 96 / 72 KB of LDS, i.e. one workgroup fewer per CU: it pays exactly when the launch cannot put a
        // second workgroup on the CUs anyway (the 7x7 layers at batch 128, most layers at small batch) and costs
        // 20-50 % otherwise (measured per layer, scripts/conv_bench.py with FQ_CONV_STAGES=2/3).
        const unsigned gy = (unsigned)(p.K / tk);
        c.stages = (sw.stages ? sw.stages == 3 : (long)gx * gy <= kCUs) ? 3 : 2;
        c.variant = c.stages == 3 ? kVarDma3 : kVarDma2;
        xcd_grid(c, gx, gy, sw);
        return c;
    }
    c.family = kFamTile;
    c.path = whole ? kPathC128 : (p.C == 64 && sw.c64 ? kPathC64 : kPathGeneral);
    c.variant = whole ? kVarTileC128 : (p.C == 64 && sw.c64 ? kVarTileC64 : kVarTileGeneral);
    xcd_grid(c, gx, (unsigned)((p.K + tk - 1) / tk), sw);
    return c;
}

}  // namespace sel
}  // namespace fq
