// fq_dwconv_dil_f32_geom.h -- the launch plan and the tile / lane -> address arithmetic of the atrous depthwise fp32 convolution
// (fq_dwconv_dil_f32.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/dwconv_dil_f32_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every global load lies
// inside x, every LDS read inside the staged rows or the zero row, and that every output element is written exactly once.
//
// A tile is PP plane slots x a band of TH output rows x TQ strips of 4 output columns (the whole output width up to 256 columns;
// wider rows are cut into CB column blocks).  Only input rows INSIDE the image are staged: for the band [oh0, oh0 + TH) the union
// over r of [oh0 - pad + r d, oh0 - pad + r d + TH) n [0, H), compacted -- R disjoint runs while TH < d, one run from TH >= d on.
// A staged row lies between zero margins (4 floats left, the row padded to a multiple of 4 plus 4 right); a tap window that
// lies wholly outside the image is read from the workgroup's one zero row instead.  The lanes walk the tile's strips, a
// strip per lane and step.
#pragma once
#include "fq_f32_geom_common.h"

namespace fq {

constexpr int kDdfBlock = 256;             // threads per workgroup
constexpr int kDdfStrip = kGeomStrip;      // output columns per strip: one 16-byte store
constexpr int kDdfMaxR = 5;
constexpr int kDdfMaxTQ = 64;              // strips per tile row: 256 output columns
constexpr int kDdfMaxPP = 32;              // plane slots per tile
constexpr int kDdfMargin = 4;              // zero floats in front of a staged row
constexpr int kDdfZero = 8;                // the zero row: LDS floats [0, 8), one window at any alignment class
constexpr int kDdfLdsFloats = 8192;        // zero row + staged input of one tile (32 KB)
constexpr int kDdfMaxBlocks = 2048;        // 256 CUs x 8 workgroups: the workgroups walk the rest of the tiles
constexpr int kDdfMaxBlocksHist = 1024;    // the histogram form flushes 2048 bins per workgroup: a smaller persistent grid

struct DdfGeom {
    int H, W, Ho, Wo, R, d, pad;
    int TQ, TH, PP;                        // strips per tile row, output rows per tile, plane slots per tile
    int RB, CB;                            // row bands x column blocks per plane
    int NR, pitch;                         // staged rows per slot (the most any tile has), their pitch in floats (a multiple of 4)
    int cls[kDdfMaxR];                     // (s d - pad) mod 4: the alignment class of tap column s's window, one for all lanes
    unsigned planes;                       // N * C
    unsigned tiles;                        // ceil(planes / PP) * RB * CB
    unsigned slot, fill;                   // NR * pitch; PP * slot = floats staged per tile (behind the zero row)
    unsigned strips;                       // PP * TH * TQ: strips per tile
    unsigned m_slot, m_pitch, m_band, m_tq;  // ceil(2^32 / .) of slot, pitch, TH * TQ, TQ: e / d = mulhi(e, m) for e * d < 2^32
};

FQ_GEOM_HD int ddf_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// in-image rows a band of th output rows touches at most: R runs of th rows while th < d, one run of th + d (R - 1) from there on
inline int ddf_band_rows(int th, int H, int R, int d) {
    const int n = th < d ? R * th : th + d * (R - 1);
    return n < H ? n : H;
}

// does the kernel take this window?  (what fq_dwconv_dil_f32_supported answers; _float_conv._dwd_ok is its Python mirror)
inline bool ddf_window_ok(int R, int d, int pad, int H, int W) {
    return (R == 3 || R == 5) && d >= 2 && d <= 64 && pad >= 0 && pad <= d * (R - 1) && H >= 1 && W >= 1 &&
           (long)H + 2 * pad >= d * (R - 1) + 1 && (long)W + 2 * pad >= d * (R - 1) + 1;
}

// The plan: a function of the layer's shape alone (never of the statistic that rides on the launch).
inline bool ddf_plan(DdfGeom& g, int N, int C, int H, int W, int R, int d, int pad) {
    if (N < 1 || C < 1 || !ddf_window_ok(R, d, pad, H, W)) return false;
    const int span = d * (R - 1);
    g.H = H; g.W = W; g.R = R; g.d = d; g.pad = pad;
    g.Ho = H + 2 * pad - span;
    g.Wo = W + 2 * pad - span;
    const int strips = (g.Wo + kDdfStrip - 1) / kDdfStrip;
    g.TQ = strips < kDdfMaxTQ ? strips : kDdfMaxTQ;
    g.CB = (strips + g.TQ - 1) / g.TQ;
    // one column block: the whole input row; else the columns under TQ strips and their taps, from a multiple of 4 on
    const int sw = g.CB == 1 ? W : g.TQ * kDdfStrip + span + 3;
    g.pitch = kDdfMargin + ((sw + 3) & ~3) + 4;
    const int nrmax = (kDdfLdsFloats - kDdfZero) / g.pitch;               // >= 15: pitch <= 524
    int th = g.Ho;
    if (ddf_band_rows(th, H, R, d) > nrmax) {
        th = nrmax - span >= d ? nrmax - span : (nrmax / R < d - 1 ? nrmax / R : d - 1);
    }
    g.TH = th;
    g.RB = (g.Ho + th - 1) / th;
    g.NR = ddf_band_rows(th, H, R, d);
    g.slot = (unsigned)(g.NR * g.pitch);
    g.planes = (unsigned)N * (unsigned)C;
    int pp = 1;
    if (g.RB == 1 && g.CB == 1 && th * g.TQ < kDdfBlock) {                // planes behind each other in x share the tile
        pp = kDdfBlock / (th * g.TQ);
        if (pp > (kDdfLdsFloats - kDdfZero) / (int)g.slot) pp = (kDdfLdsFloats - kDdfZero) / (int)g.slot;
        if (pp > kDdfMaxPP) pp = kDdfMaxPP;
        if ((unsigned)pp > g.planes) pp = (int)g.planes;
    }
    g.PP = pp;
    g.fill = (unsigned)pp * g.slot;
    g.strips = (unsigned)(pp * th * g.TQ);
    g.tiles = ((g.planes + (unsigned)pp - 1u) / (unsigned)pp) * (unsigned)(g.RB * g.CB);
    for (int s = 0; s < kDdfMaxR; ++s) g.cls[s] = ((s * d - pad) % 4 + 4) % 4;
    g.m_slot = 0xffffffffu / g.slot + 1u;
    g.m_pitch = 0xffffffffu / (unsigned)g.pitch + 1u;
    g.m_band = 0xffffffffu / (unsigned)(th * g.TQ) + 1u;
    g.m_tq = 0xffffffffu / (unsigned)g.TQ + 1u;
    return true;
}

inline unsigned ddf_grid(const DdfGeom& g, bool hist) {
    const unsigned cap = hist ? (unsigned)kDdfMaxBlocksHist : (unsigned)kDdfMaxBlocks;
    return g.tiles < cap ? g.tiles : cap;
}

// tile -> first plane, first output row and column, first staged input column (a multiple of 4), and the staged runs of rows:
// run r holds the in-image rows of [oh0 - pad + r d, + TH) that no earlier run holds, in slot rows [base[r], base[r + 1]);
// input row ih of run r is slot row ih + off[r] -- also where run r is empty because an earlier run holds its rows (TH >= d)
struct DdfTilePos {
    unsigned plane0;
    int oh0, ow0, cb0;
    int base[kDdfMaxR + 1], off[kDdfMaxR];
};
FQ_GEOM_HD DdfTilePos ddf_tile_pos(const DdfGeom& g, unsigned tile) {
    DdfTilePos t;
    const unsigned per = (unsigned)(g.RB * g.CB), grp = tile / per, rest = tile - grp * per;
    const unsigned rb = rest / (unsigned)g.CB, cb = rest - rb * (unsigned)g.CB;
    t.plane0 = grp * (unsigned)g.PP;
    t.oh0 = (int)rb * g.TH;
    t.ow0 = (int)cb * g.TQ * kDdfStrip;
    t.cb0 = g.CB == 1 || t.ow0 < g.pad ? 0 : (t.ow0 - g.pad) & ~3;
    int prev = 0, base = 0;
    for (int r = 0; r < kDdfMaxR; ++r) {
        const int a = t.oh0 - g.pad + r * g.d;
        int lo = r < g.R ? ddf_clamp(a, 0, g.H) : prev, hi = r < g.R ? ddf_clamp(a + g.TH, 0, g.H) : prev;
        if (lo < prev) lo = prev;
        if (hi < lo) hi = lo;
        t.base[r] = base;
        t.off[r] = base - lo;
        base += hi - lo;
        prev = hi;
    }
    t.base[kDdfMaxR] = base;
    return t;
}

// Staging: LDS float kDdfZero + e of the tile <- input pixel (plane0 + pi, row of slot row sr, cb0 + col - 4), or +0.0f where
// that is no pixel (the margins, slot rows the tile does not use, slots behind the last plane).  Returns whether it is a load;
// *off is then its element offset into x.
FQ_GEOM_HD bool ddf_fill_src(const DdfGeom& g, const DdfTilePos& tp, unsigned e, unsigned* off) {
    const unsigned pi = geom_mulhi(e, g.m_slot), rem = e - pi * g.slot;
    const unsigned sr = geom_mulhi(rem, g.m_pitch), col = rem - sr * (unsigned)g.pitch;
    int ih = -1;
    for (int r = 0; r < kDdfMaxR; ++r)
        if ((int)sr >= tp.base[r] && (int)sr < tp.base[r + 1]) ih = (int)sr - tp.off[r];
    const int iw = tp.cb0 + (int)col - kDdfMargin;
    const unsigned plane = tp.plane0 + pi;
    const bool ok = plane < g.planes && ih >= 0 && (unsigned)iw < (unsigned)g.W;
    *off = ok ? (plane * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw : 0u;
    return ok;
}

// strip u of a tile -> (plane slot, output row of the band, strip of that row)
struct DdfStripPos { int pi, t, q; };
FQ_GEOM_HD DdfStripPos ddf_strip_pos(const DdfGeom& g, unsigned u) {
    DdfStripPos l;
    // (ceil(2^32 / 1) does not fit 32 bits: a divisor of 1 is the identity)
    const unsigned band = (unsigned)(g.TH * g.TQ);
    const unsigned pi = band == 1u ? u : geom_mulhi(u, g.m_band), rem = u - pi * band;
    const unsigned t = g.TQ == 1 ? rem : geom_mulhi(rem, g.m_tq);
    l.pi = (int)pi; l.t = (int)t; l.q = (int)(rem - t * (unsigned)g.TQ);
    return l;
}

// the staged row under band row t for kernel row r: its float offset inside the slot, or -1 for a row outside the image
FQ_GEOM_HD int ddf_row_off(const DdfGeom& g, const DdfTilePos& tp, int t, int r) {
    const int ih = tp.oh0 + t - g.pad + r * g.d;
    return (unsigned)ih < (unsigned)g.H ? (ih + tp.off[r]) * g.pitch : -1;
}

// the 4 floats strip q reads for tap column s: their first column inside a staged row, or -1 where the whole window lies
// outside the image (a window that hangs over an edge reads the row's zero margin)
FQ_GEOM_HD int ddf_win_col(const DdfGeom& g, const DdfTilePos& tp, int q, int s) {
    const int c = tp.ow0 + q * kDdfStrip - g.pad + s * g.d;
    return c + (kDdfStrip - 1) >= 0 && c < g.W ? kDdfMargin + c - tp.cb0 : -1;
}

// the LDS float a tap's window starts at: a lane selects an address, never a value
FQ_GEOM_HD unsigned ddf_read_index(const DdfGeom& g, int pi, int row_off, int win_col, int s) {
    return row_off >= 0 && win_col >= 0 ? (unsigned)kDdfZero + (unsigned)pi * g.slot + (unsigned)(row_off + win_col)
                                        : (unsigned)g.cls[s];
}

// the strip in y: how many of its 4 outputs exist (0: none), and the element offset of the first
FQ_GEOM_HD int ddf_out_count(const DdfGeom& g, const DdfTilePos& tp, const DdfStripPos& l) {
    const int oh = tp.oh0 + l.t, ow = tp.ow0 + l.q * kDdfStrip;
    if (tp.plane0 + (unsigned)l.pi >= g.planes || oh >= g.Ho || ow >= g.Wo) return 0;
    return g.Wo - ow < kDdfStrip ? g.Wo - ow : kDdfStrip;
}
FQ_GEOM_HD unsigned ddf_out_off(const DdfGeom& g, const DdfTilePos& tp, const DdfStripPos& l) {
    return ((tp.plane0 + (unsigned)l.pi) * (unsigned)g.Ho + (unsigned)(tp.oh0 + l.t)) * (unsigned)g.Wo +
           (unsigned)(tp.ow0 + l.q * kDdfStrip);
}

}  // namespace fq
