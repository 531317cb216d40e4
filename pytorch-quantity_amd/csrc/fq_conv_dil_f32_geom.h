// fq_conv_dil_f32_geom.h -- the launch plan and the tile / lane -> address arithmetic of the atrous dense 3x3 fp32 convolution
// (fq_conv_dil_f32.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/conv_dil_f32_geom_check.cpp walks them over the shapes the GPU tests run and the model's layers and asserts that every
// staged element comes from inside x, every LDS read lies in the staged pixels or the zero pixel, every live tap reads the float
// staged from its pixel, every culled tap is dead for every pixel of its tile, and every output is written exactly once.
//
// A tile is 32 MT output channels x a rectangle of TH x TW output pixels of one image (TH TW <= 128: a pixel per lane of the four
// waves).  Both axes are treated alike (CdAxis): tap r of an axis needs the inputs [o0 - pad + r d, o0 - pad + r d + len) n [0, L);
// it is LIVE iff that is not empty, the in-image inputs of the three taps are staged compacted -- slot = input + off[r]; three
// disjoint runs while len < d, merged runs from len >= d on -- and nothing outside the image is staged at all.  A staged pixel
// is kCdChunk channels behind each other at a pitch of kCdPitch floats (odd: neighbouring pixels fall into neighbouring banks,
// for the staging stores and for the operand reads alike).  A tap whose source pixel lies outside the image reads the zero
// pixel at LDS float 0: a lane selects an address, never a value.
#pragma once
#include "fq_f32_geom_common.h"

namespace fq {

constexpr int kCdBlock = 256;              // threads per workgroup: 4 waves
constexpr int kCdChunk = 8;                // input channels per staged chunk = FQ_CONV_DIL_F32_CHUNK (include/fq.h): 4 MFMA k steps
constexpr int kCdPitch = kCdChunk + 1;     // floats between staged pixels
constexpr int kCdZero = 16;                // LDS floats [0, 16): the zero pixel
constexpr int kCdTilePx = 128;             // output pixels per tile at most: 32 per wave
constexpr int kCdMaxTW = 32;               // output columns per tile at most
constexpr int kCdMaxPx = 896;              // staged pixels per tile at most (31.5 KB a chunk)
constexpr int kCdPxPerThread = (kCdMaxPx + kCdBlock - 1) / kCdBlock;
constexpr int kCdMaxBlocks = 2048;         // 256 CUs x 8 workgroups: the workgroups walk the rest of the tiles
constexpr int kCdMaxBlocksHist = 1024;     // the histogram form flushes 2048 bins per workgroup: a smaller persistent grid
constexpr int kCdFewTiles = 512;           // fewer 64-channel tiles than this: 32-channel tiles instead

struct CdGeom {
    int N, Cin, Cout, H, W, Ho, Wo, d, pad;
    int MT;                                // 32-channel accumulator tiles per wave: 1 or 2
    int TH, TW;                            // output rows and columns per tile
    int MB, RB, CB;                        // channel blocks, row bands and column blocks per image
    unsigned tiles;                        // N * RB * CB * MB
};

FQ_GEOM_HD int cd_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// in-image inputs `len` neighbouring outputs touch along one axis at most
inline int cd_axis_max(int len, int L, int d) {
    const int n = len < d ? 3 * len : len + 2 * d;
    return n < L ? n : L;
}

// does the kernel take this layer?  (what fq_conv_dil_f32_supported answers; _float_conv._kd_ok is its Python mirror)
inline bool cd_supported(int Cin, int Cout, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                         int dil_w, int H, int W) {
    return groups == 1 && R == 3 && S == 3 && stride_h == 1 && stride_w == 1 && dil_h == dil_w && pad_h == pad_w && dil_h >= 2 &&
           dil_h <= 64 && pad_h >= 0 && pad_h <= 2 * dil_h && Cin >= 16 && Cin % 16 == 0 && Cout >= 4 && Cout % 4 == 0 && H >= 1 &&
           W >= 1 && (long)H + 2 * pad_h >= 2 * dil_h + 1 && (long)W + 2 * pad_h >= 2 * dil_h + 1;
}

// The plan: a function of the layer's shape alone (never of the statistic that rides on the launch).
inline bool cd_plan(CdGeom& g, int N, int Cin, int Cout, int H, int W, int d, int pad) {
    if (N < 1 || !cd_supported(Cin, Cout, 1, 3, 3, 1, 1, pad, pad, d, d, H, W)) return false;
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.H = H; g.W = W; g.d = d; g.pad = pad;
    g.Ho = H + 2 * pad - 2 * d;
    g.Wo = W + 2 * pad - 2 * d;
    g.TW = g.Wo < kCdMaxTW ? g.Wo : kCdMaxTW;
    int th = kCdTilePx / g.TW;
    if (th > g.Ho) th = g.Ho;
    while (th > 1 && cd_axis_max(th, H, d) * cd_axis_max(g.TW, W, d) > kCdMaxPx) --th;      // (32 columns at d > 4: 3 rows, 96 of 128 lanes)
    if (cd_axis_max(th, H, d) * cd_axis_max(g.TW, W, d) > kCdMaxPx) return false;            // (3 x 96 at most: never)
    g.TH = th;
    g.RB = (g.Ho + th - 1) / th;
    g.CB = (g.Wo + g.TW - 1) / g.TW;
    const long px_tiles = (long)N * g.RB * g.CB;
    g.MT = Cout > 32 && px_tiles * ((Cout + 63) / 64) >= kCdFewTiles ? 2 : 1;
    g.MB = (Cout + 32 * g.MT - 1) / (32 * g.MT);
    if (px_tiles * g.MB >= (1L << 31)) return false;
    g.tiles = (unsigned)(px_tiles * g.MB);
    return true;
}

inline unsigned cd_grid(const CdGeom& g, bool hist) {
    const unsigned cap = hist ? (unsigned)kCdMaxBlocksHist : (unsigned)kCdMaxBlocks;
    return g.tiles < cap ? g.tiles : cap;
}

// one axis of a tile: which of the three taps are live, and where their in-image inputs are staged.  Run r holds the inputs of
// [o0 - pad + r d, + len) n [0, L) that no earlier run holds, in slots [base[r], base[r + 1]); input i of tap r is slot
// i + off[r] -- also where an earlier run holds it (len >= d: the merged runs share one off)
struct CdAxis {
    int base[4], off[3];
    int live;                              // bit r: tap r has a source inside [0, L) for some output of the tile
};
FQ_GEOM_HD CdAxis cd_axis(int o0, int len, int pad, int d, int L) {
    CdAxis a;
    a.live = 0;
    int prev = 0, base = 0;
    for (int r = 0; r < 3; ++r) {
        const int first = o0 - pad + r * d;
        int lo = cd_clamp(first, 0, L), hi = cd_clamp(first + len, 0, L);
        if (hi > lo) a.live |= 1 << r;
        if (lo < prev) lo = prev;
        if (hi < lo) hi = lo;
        a.base[r] = base;
        a.off[r] = base - lo;
        base += hi - lo;
        prev = hi;
    }
    a.base[3] = base;
    return a;
}
// slot -> the input it holds (slot < base[3])
FQ_GEOM_HD int cd_axis_input(const CdAxis& a, int slot) {
    int i = 0;
    for (int r = 0; r < 3; ++r)
        if (slot >= a.base[r] && slot < a.base[r + 1]) i = slot - a.off[r];
    return i;
}

// tile -> image, first output channel, the rectangle [p0, p0 + th) x [q0, q0 + tw) and its two axes (channel block fastest: the
// workgroups that run together read the same pixels of x)
struct CdTilePos {
    unsigned n, m0;
    int p0, q0, th, tw;
    CdAxis rows, cols;
    unsigned staged;                       // rows.base[3] * cols.base[3] pixels
};
FQ_GEOM_HD CdTilePos cd_tile_pos(const CdGeom& g, unsigned tile) {
    CdTilePos t;
    const unsigned mb = tile % (unsigned)g.MB, rest = tile / (unsigned)g.MB;
    const unsigned cb = rest % (unsigned)g.CB, rest2 = rest / (unsigned)g.CB;
    const unsigned rb = rest2 % (unsigned)g.RB;
    t.n = rest2 / (unsigned)g.RB;
    t.m0 = mb * 32u * (unsigned)g.MT;
    t.p0 = (int)rb * g.TH;
    t.q0 = (int)cb * g.TW;
    t.th = g.Ho - t.p0 < g.TH ? g.Ho - t.p0 : g.TH;
    t.tw = g.Wo - t.q0 < g.TW ? g.Wo - t.q0 : g.TW;
    t.rows = cd_axis(t.p0, t.th, g.pad, g.d, g.H);
    t.cols = cd_axis(t.q0, t.tw, g.pad, g.d, g.W);
    t.staged = (unsigned)(t.rows.base[3] * t.cols.base[3]);
    return t;
}

// Staging: staged pixel px (< tp.staged; LDS floats kCdZero + px kCdPitch + c for the chunk's channels c) <- x[n][c0 + c][ih][iw];
// returns ih W + iw.  Every staged pixel lies inside the image: there is nothing to predicate but px < staged.
FQ_GEOM_HD unsigned cd_stage_src(const CdGeom& g, const CdTilePos& tp, unsigned px) {
    const unsigned sc = (unsigned)tp.cols.base[3], sr = px / sc;
    return (unsigned)cd_axis_input(tp.rows, (int)sr) * (unsigned)g.W + (unsigned)cd_axis_input(tp.cols, (int)(px - sr * sc));
}
// element offset of x[n][c][0][0]
FQ_GEOM_HD unsigned cd_x_plane(const CdGeom& g, unsigned n, unsigned c) { return (n * (unsigned)g.Cin + c) * (unsigned)(g.H * g.W); }

// lane j (0 .. 127: 32 wave + lane % 32) of a tile -> its output pixel; false where the lane has none
struct CdLanePos { int p, q; };
FQ_GEOM_HD bool cd_lane_pos(const CdGeom& g, const CdTilePos& tp, unsigned j, CdLanePos* l) {
    const unsigned t = j / (unsigned)g.TW, u = j - t * (unsigned)g.TW;
    l->p = tp.p0 + (int)t;
    l->q = tp.q0 + (int)u;
    return (int)t < tp.th && (int)u < tp.tw;
}
// the LDS float the lane's operand for tap (r, s) and channel 0 of the chunk lies at: its staged pixel, or the zero pixel
FQ_GEOM_HD unsigned cd_read_index(const CdGeom& g, const CdTilePos& tp, bool has, const CdLanePos& l, int r, int s) {
    const int ih = l.p - g.pad + r * g.d, iw = l.q - g.pad + s * g.d;
    const bool in = has && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
    return in ? (unsigned)kCdZero + (unsigned)((ih + tp.rows.off[r]) * tp.cols.base[3] + iw + tp.cols.off[s]) * (unsigned)kCdPitch : 0u;
}
// a wave with no pixel in the tile skips the K loop
FQ_GEOM_HD bool cd_wave_active(const CdGeom& g, const CdTilePos& tp, unsigned wave) { return wave * 32u < (unsigned)(tp.th * g.TW); }

// accumulator register e of half-wave h -> channel row of the 32 x 32 MFMA tile
FQ_GEOM_HD unsigned cd_acc_row(int e, unsigned h) { return (unsigned)((e & 3) + 8 * (e >> 2)) + 4u * h; }
FQ_GEOM_HD unsigned cd_out_off(const CdGeom& g, unsigned n, unsigned k, const CdLanePos& l) {
    return ((n * (unsigned)g.Cout + k) * (unsigned)g.Ho + (unsigned)l.p) * (unsigned)g.Wo + (unsigned)l.q;
}

}  // namespace fq
