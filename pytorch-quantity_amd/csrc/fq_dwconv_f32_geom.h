// fq_dwconv_f32_geom.h -- the launch plan and the tile / lane -> address arithmetic of the depthwise fp32 convolution
// (fq_dwconv_f32.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/dwconv_f32_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every global load lies
// inside x, every LDS index inside the staged tile, every store inside y, and every output element is written exactly once.
//
// A tile is PP plane slots of TH output rows x 4 QW output columns; a lane owns one 1 x 4 output strip of one slot.  Each slot's
// input rows (IH of them, zero halo included) are staged in LDS with the pitch IWP.  A plane that fits one tile shares the
// tile with the PP - 1 planes behind it (they are contiguous in NCHW: 18 planes of 7 x 7 per tile); a larger plane is cut
// into RB row bands x CB column blocks and PP is 1.
#pragma once
#include "fq_f32_geom_common.h"

namespace fq {

constexpr int kDwfBlock = 256;             // threads per workgroup = output strips per tile
constexpr int kDwfStrip = kGeomStrip;              // output columns per lane: one 16-byte store
constexpr int kDwfMaxQW = 16;              // strips per tile row: 64 output columns
constexpr int kDwfMaxPP = 32;              // plane slots per tile
constexpr int kDwfLdsFloats = 5120;        // staged input of one tile (20 KB)
constexpr int kDwfMaxBlocks = 2048;        // 256 CUs x 8 workgroups: the workgroups walk the rest of the tiles
constexpr int kDwfMaxBlocksHist = 1024;    // the histogram form flushes 2048 bins per workgroup: a smaller persistent grid

struct DwfGeom {
    int H, W, Ho, Wo, stride, pad;
    int QW, TH, PP;                        // strips per tile row, output rows per tile, plane slots per tile
    int IH, IWP;                           // staged input rows per slot, their pitch in floats (a multiple of 4)
    int RB, CB;                            // row bands x column blocks per plane
    unsigned planes;                       // N * C
    unsigned tiles;                        // ceil(planes / PP) * RB * CB
    unsigned slot, fill;                   // IH * IWP; PP * slot = floats staged per tile
    unsigned m_slot, m_pitch;              // ceil(2^32 / slot), ceil(2^32 / IWP): e / d = mulhi(e, m) for e * d < 2^32
};

// The plan: a function of the layer's shape alone (never of the statistic that rides on the launch).
inline bool dwf_plan(DwfGeom& g, int N, int C, int H, int W, int R, int stride, int pad) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || (R != 3 && R != 5) || (stride != 1 && stride != 2) || pad < 0 || pad >= R ||
        H + 2 * pad < R || W + 2 * pad < R)
        return false;
    g.H = H; g.W = W; g.stride = stride; g.pad = pad;
    g.Ho = (H + 2 * pad - R) / stride + 1;
    g.Wo = (W + 2 * pad - R) / stride + 1;
    const int strips = (g.Wo + kDwfStrip - 1) / kDwfStrip;
    g.QW = strips < kDwfMaxQW ? strips : kDwfMaxQW;
    g.CB = (strips + g.QW - 1) / g.QW;
    g.IWP = (g.QW - 1) * kDwfStrip * stride + 4 * geom_strip_reads(R, stride);
    int th = kDwfBlock / g.QW;
    const int th_lds = (kDwfLdsFloats / g.IWP - R) / stride + 1;          // ((TH - 1) stride + R) IWP <= kDwfLdsFloats
    if (th > th_lds) th = th_lds;
    if (th > g.Ho) th = g.Ho;
    g.TH = th;
    g.RB = (g.Ho + th - 1) / th;
    g.IH = (th - 1) * stride + R;
    g.slot = (unsigned)(g.IH * g.IWP);
    g.planes = (unsigned)N * (unsigned)C;
    int pp = 1;
    if (g.RB == 1 && g.CB == 1) {
        pp = kDwfBlock / (g.TH * g.QW);
        if (pp > kDwfLdsFloats / (int)g.slot) pp = kDwfLdsFloats / (int)g.slot;
        if (pp > kDwfMaxPP) pp = kDwfMaxPP;
        if ((unsigned)pp > g.planes) pp = (int)g.planes;
    }
    g.PP = pp;
    g.fill = (unsigned)pp * g.slot;
    g.tiles = ((g.planes + (unsigned)pp - 1u) / (unsigned)pp) * (unsigned)(g.RB * g.CB);
    g.m_slot = 0xffffffffu / g.slot + 1u;
    g.m_pitch = 0xffffffffu / (unsigned)g.IWP + 1u;
    return true;
}

inline unsigned dwf_grid(const DwfGeom& g, bool hist) {
    const unsigned cap = hist ? (unsigned)kDwfMaxBlocksHist : (unsigned)kDwfMaxBlocks;
    return g.tiles < cap ? g.tiles : cap;
}

// tile -> first plane, first output row, first output column (column block fastest, then row band, then plane group)
struct DwfTilePos { unsigned plane0; int oh0, ow0; };
FQ_GEOM_HD DwfTilePos dwf_tile_pos(const DwfGeom& g, unsigned tile) {
    DwfTilePos t;
    const unsigned per = (unsigned)(g.RB * g.CB), grp = tile / per, rest = tile - grp * per;
    const unsigned rb = rest / (unsigned)g.CB, cb = rest - rb * (unsigned)g.CB;
    t.plane0 = grp * (unsigned)g.PP;
    t.oh0 = (int)rb * g.TH;
    t.ow0 = (int)cb * g.QW * kDwfStrip;
    return t;
}

// lane -> (plane slot, output row of the tile, strip of that row); the same for every tile of a launch
struct DwfLanePos { int pi, t, q; bool active; };
FQ_GEOM_HD DwfLanePos dwf_lane_pos(const DwfGeom& g, unsigned tid) {
    DwfLanePos l;
    const unsigned per = (unsigned)(g.TH * g.QW);
    l.pi = (int)(tid / per);
    const unsigned rem = tid - (unsigned)l.pi * per;
    l.t = (int)(rem / (unsigned)g.QW);
    l.q = (int)(rem - (unsigned)l.t * (unsigned)g.QW);
    l.active = l.pi < g.PP;
    return l;
}

// Staging: LDS float e of the tile <- input pixel (plane0 + pi, ih0 + r, iw0 + col), or +0.0f outside the image (and behind
// the last plane).  Returns whether it is a load; *off is then its element offset into x.
FQ_GEOM_HD bool dwf_fill_src(const DwfGeom& g, const DwfTilePos& tp, unsigned e, unsigned* off) {
    const unsigned pi = geom_mulhi(e, g.m_slot), rem = e - pi * g.slot;
    const unsigned r = geom_mulhi(rem, g.m_pitch), col = rem - r * (unsigned)g.IWP;
    const int ih = tp.oh0 * g.stride - g.pad + (int)r, iw = tp.ow0 * g.stride - g.pad + (int)col;
    const unsigned plane = tp.plane0 + pi;
    const bool ok = plane < g.planes && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
    *off = ok ? (plane * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw : 0u;
    return ok;
}

// first LDS float of the lane's strip in staged row 0 of its window (kernel row r adds r * IWP); 16-byte aligned
FQ_GEOM_HD unsigned dwf_read_index(const DwfGeom& g, const DwfLanePos& l) {
    return (unsigned)l.pi * g.slot + (unsigned)(l.t * g.stride * g.IWP + l.q * kDwfStrip * g.stride);
}

// the lane's strip in y: how many of its 4 outputs exist (0: none), and the element offset of the first
FQ_GEOM_HD int dwf_out_count(const DwfGeom& g, const DwfTilePos& tp, const DwfLanePos& l) {
    const int oh = tp.oh0 + l.t, ow = tp.ow0 + l.q * kDwfStrip;
    if (!l.active || tp.plane0 + (unsigned)l.pi >= g.planes || oh >= g.Ho || ow >= g.Wo) return 0;
    return g.Wo - ow < kDwfStrip ? g.Wo - ow : kDwfStrip;
}
FQ_GEOM_HD unsigned dwf_out_off(const DwfGeom& g, const DwfTilePos& tp, const DwfLanePos& l) {
    return ((tp.plane0 + (unsigned)l.pi) * (unsigned)g.Ho + (unsigned)(tp.oh0 + l.t)) * (unsigned)g.Wo +
           (unsigned)(tp.ow0 + l.q * kDwfStrip);
}

}  // namespace fq
