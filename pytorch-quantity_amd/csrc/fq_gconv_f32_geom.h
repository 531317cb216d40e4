// fq_gconv_f32_geom.h -- the launch plan and the tile / lane -> address arithmetic of the grouped fp32 convolution
// (fq_gconv_f32.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/gconv_f32_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every global load lies
// inside x or w, every LDS index inside the staged tile, every store inside y, and every output element is written exactly once.
//
// A tile is one (image, group, chunk of KC output channels, row band, column block): TH output rows x QW strips of 4 output
// columns x KBN blocks of 4 output channels; a lane owns one strip of one channel block (16 accumulators).  LDS holds the
// chunk's weights as [tap][c][KC] (a lane reads its 4 channels of one (tap, c) as one 16-byte read), the chunk's bias, and in
// everything that is left the group's Cgi input windows (IH rows of pitch IWP each, zero halo included) one behind the other:
// a group of few channels gets tall tiles, a group of many channels still gets its 4096 floats.
#pragma once
#include "fq_f32_geom_common.h"

namespace fq {

constexpr int kGfBlock = 256;              // threads per workgroup
constexpr int kGfStrip = kGeomStrip;               // output columns per lane: one 16-byte store per channel
constexpr int kGfKB = 4;                   // output channels per lane: one 16-byte weight read per (tap, c)
constexpr int kGfMaxQW = 16;               // strips per tile row: 64 output columns
constexpr int kGfMaxKC = 64;               // output channels per tile
constexpr int kGfWFloats = 9216;           // staged weights of one tile, at most (36 KB): 32 x 32 x 9, or 16 channels of 64 x 9
constexpr int kGfLdsFloats = 13376;        // weights + bias + staged input of one tile (52.25 KB: three workgroups per CU)
constexpr int kGfMinInFloats = kGfLdsFloats - kGfMaxKC - kGfWFloats;   // 4096: what the input has whatever the weights take
constexpr int kGfMaxBlocks = 2048;         // 256 CUs x 8 workgroups: the workgroups walk the rest of the tiles
constexpr int kGfMaxBlocksHist = 1024;     // the histogram form flushes 2048 bins per workgroup: a smaller persistent grid

struct GfGeom {
    int H, W, Ho, Wo, stride, pad, R, RR;
    int C, K, G, Cgi, Cgo;
    int KC, KCN, KBN;                      // output channels per chunk, chunks per group, 4-channel blocks per chunk
    int QW, TH;                            // strips per tile row, output rows per tile
    int IH, IWP;                           // staged input rows per channel, their pitch in floats (a multiple of 4)
    int RB, CB;                            // row bands x column blocks per plane
    unsigned units;                        // N * G
    unsigned tiles;                        // units * KCN * RB * CB
    unsigned slot, fill;                   // IH * IWP; Cgi * slot = input floats staged per tile
    unsigned ckr, wfill;                   // Cgi * RR = weights per output channel; KC * ckr = weight floats staged per tile
    unsigned b0, x0, in_floats;            // LDS float offsets of the bias (= wfill) and of the input; floats the input may take
    unsigned m_slot, m_pitch, m_ckr, m_rr; // ceil(2^32 / d) of slot, IWP, ckr, RR: e / d = mulhi(e, m) for e * d < 2^32
};

inline bool gf_supported(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                         int dil_w, int H, int W) {
    if (groups < 2 || C < 1 || K < 1 || H < 1 || W < 1 || C % groups || K % groups) return false;
    const int cgi = C / groups, cgo = K / groups;
    return cgi % 4 == 0 && cgo % 4 == 0 && cgi >= 4 && cgi <= 64 && cgo >= 4 && cgo <= 64 && R == S && (R == 1 || R == 3) &&
           stride_h == stride_w && (stride_h == 1 || stride_h == 2) && dil_h == 1 && dil_w == 1 && pad_h == pad_w && pad_h >= 0 &&
           pad_h < R && H + 2 * pad_h >= R && W + 2 * pad_w >= S;
}

// The plan: a function of the layer's shape alone (never of the statistic that rides on the launch).
inline bool gf_plan(GfGeom& g, int N, int C, int H, int W, int K, int groups, int R, int stride, int pad) {
    if (N < 1 || !gf_supported(C, K, groups, R, R, stride, stride, pad, pad, 1, 1, H, W)) return false;
    g.H = H; g.W = W; g.stride = stride; g.pad = pad; g.R = R; g.RR = R * R;
    g.C = C; g.K = K; g.G = groups; g.Cgi = C / groups; g.Cgo = K / groups;
    g.Ho = (H + 2 * pad - R) / stride + 1;
    g.Wo = (W + 2 * pad - R) / stride + 1;
    g.ckr = (unsigned)(g.Cgi * g.RR);
    const int kcmax = (kGfWFloats / (int)g.ckr) & ~3;                     // >= 16: 64 * 9 * 16 = kGfWFloats
    g.KCN = (g.Cgo + kcmax - 1) / kcmax;
    g.KC = (((g.Cgo + g.KCN - 1) / g.KCN) + 3) & ~3;
    g.KBN = g.KC / kGfKB;
    g.wfill = (unsigned)g.KC * g.ckr;
    g.b0 = g.wfill;
    g.x0 = g.wfill + (unsigned)kGfMaxKC;
    g.in_floats = (unsigned)kGfLdsFloats - g.x0;                          // >= kGfMinInFloats
    const int slot_max = (int)g.in_floats / g.Cgi;                        // >= 64
    const int strips = (g.Wo + kGfStrip - 1) / kGfStrip, nrd = geom_strip_reads(R, stride);
    // every width of a column block: the blocks made evenly wide and the row bands evenly tall, then the widest one, unless a
    // narrower one keeps 15 % more lanes busy (a wide tile stores long row segments)
    int best = 0;
    for (int qw0 = strips < kGfMaxQW ? strips : kGfMaxQW; qw0 >= 1; --qw0) {
        const int cb = (strips + qw0 - 1) / qw0, qw = (strips + cb - 1) / cb;
        const int iwp = (qw - 1) * kGfStrip * stride + 4 * nrd;
        if (slot_max / iwp < R) continue;
        int th = kGfBlock / (qw * g.KBN);
        const int th_lds = (slot_max / iwp - R) / stride + 1;             // ((TH - 1) stride + R) IWP <= slot_max
        if (th > th_lds) th = th_lds;
        if (th > g.Ho) th = g.Ho;
        if (th < 1) continue;
        const int rb = (g.Ho + th - 1) / th, thb = (g.Ho + rb - 1) / rb;
        if (20 * qw * thb > 23 * best) { best = qw * thb; g.QW = qw; g.CB = cb; g.TH = thb; g.RB = rb; }
    }
    if (best < 1) return false;
    g.IWP = (g.QW - 1) * kGfStrip * stride + 4 * nrd;
    g.IH = (g.TH - 1) * stride + R;
    g.slot = (unsigned)(g.IH * g.IWP);
    g.fill = (unsigned)g.Cgi * g.slot;
    g.units = (unsigned)N * (unsigned)groups;
    g.tiles = g.units * (unsigned)(g.KCN * g.RB * g.CB);
    g.m_slot = 0xffffffffu / g.slot + 1u;
    g.m_pitch = 0xffffffffu / (unsigned)g.IWP + 1u;
    g.m_ckr = 0xffffffffu / g.ckr + 1u;
    g.m_rr = g.RR == 1 ? 0u : 0xffffffffu / (unsigned)g.RR + 1u;          // (unused for a 1x1 kernel)
    return true;
}

inline unsigned gf_grid(const GfGeom& g, bool hist) {
    const unsigned cap = hist ? (unsigned)kGfMaxBlocksHist : (unsigned)kGfMaxBlocks;
    return g.tiles < cap ? g.tiles : cap;
}

// tile -> image, group, first output channel of the chunk (within the group), first output row, first output column
// (column block fastest, then row band, then channel chunk, then group, then image)
struct GfTilePos { unsigned n, grp; int k0, oh0, ow0; };
FQ_GEOM_HD GfTilePos gf_tile_pos(const GfGeom& g, unsigned tile) {
    GfTilePos t;
    const unsigned sp = (unsigned)(g.RB * g.CB), per = (unsigned)g.KCN * sp;
    const unsigned u = tile / per, rest = tile - u * per;
    const unsigned kc = rest / sp, rest2 = rest - kc * sp;
    const unsigned rb = rest2 / (unsigned)g.CB, cb = rest2 - rb * (unsigned)g.CB;
    t.n = u / (unsigned)g.G;
    t.grp = u - t.n * (unsigned)g.G;
    t.k0 = (int)kc * g.KC;
    t.oh0 = (int)rb * g.TH;
    t.ow0 = (int)cb * g.QW * kGfStrip;
    return t;
}

// lane -> (channel block of the chunk, output row of the tile, strip of that row); the same for every tile of a launch
struct GfLanePos { int kb, t, q; bool active; };
FQ_GEOM_HD GfLanePos gf_lane_pos(const GfGeom& g, unsigned tid) {
    GfLanePos l;
    const unsigned per = (unsigned)(g.TH * g.QW);
    l.kb = (int)(tid / per);
    const unsigned rem = tid - (unsigned)l.kb * per;
    l.t = (int)(rem / (unsigned)g.QW);
    l.q = (int)(rem - (unsigned)l.t * (unsigned)g.QW);
    l.active = l.kb < g.KBN;
    return l;
}

// Input staging: LDS float e (< fill) of the tile <- input pixel (n, grp * Cgi + c, ih0 + r, iw0 + col), or +0.0f outside the
// image.  Returns whether it is a load; *off is then its element offset into x.
FQ_GEOM_HD bool gf_fill_src(const GfGeom& g, const GfTilePos& tp, unsigned e, unsigned* off) {
    const unsigned c = geom_mulhi(e, g.m_slot), rem = e - c * g.slot;
    const unsigned r = geom_mulhi(rem, g.m_pitch), col = rem - r * (unsigned)g.IWP;
    const int ih = tp.oh0 * g.stride - g.pad + (int)r, iw = tp.ow0 * g.stride - g.pad + (int)col;
    const bool ok = (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
    const unsigned plane = tp.n * (unsigned)g.C + tp.grp * (unsigned)g.Cgi + c;
    *off = ok ? (plane * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw : 0u;
    return ok;
}

// Weight staging: element i (< wfill) of the chunk's run of w_kcrs -- (kk, c, tap), the module's own order -- goes to the LDS
// weight float *dst = (tap * Cgi + c) * KC + kk.  Returns whether it is a load (a channel behind the group's last is +0.0f);
// *off is then its element offset into w.
FQ_GEOM_HD bool gf_w_src(const GfGeom& g, const GfTilePos& tp, unsigned i, unsigned* off, unsigned* dst) {
    const unsigned kk = geom_mulhi(i, g.m_ckr), rem = i - kk * g.ckr;
    const unsigned c = g.RR == 1 ? rem : geom_mulhi(rem, g.m_rr), tap = rem - c * (unsigned)g.RR;     // (2^32 / 1 has no 32-bit form)
    *dst = (tap * (unsigned)g.Cgi + c) * (unsigned)g.KC + kk;
    const bool ok = tp.k0 + (int)kk < g.Cgo;
    *off = ok ? (tp.grp * (unsigned)g.Cgo + (unsigned)tp.k0) * g.ckr + i : 0u;
    return ok;
}

// first float of the lane's strip in staged row 0 of channel 0, counted from the input's LDS offset x0 (channel c adds
// c * slot, kernel row r adds r * IWP); 16-byte aligned
FQ_GEOM_HD unsigned gf_read_index(const GfGeom& g, const GfLanePos& l) {
    return (unsigned)(l.t * g.stride * g.IWP + l.q * kGfStrip * g.stride);
}
// the lane's 4 weights of (tap, c) in the LDS weight block; 16-byte aligned
FQ_GEOM_HD unsigned gf_w_index(const GfGeom& g, const GfLanePos& l, int tap, int c) {
    return (unsigned)((tap * g.Cgi + c) * g.KC + l.kb * kGfKB);
}

// the lane's strip in y: how many of its 4 columns exist (0: none; its 4 channels exist together or not at all), and the
// element offset of the first column of channel kk of its block
FQ_GEOM_HD int gf_out_count(const GfGeom& g, const GfTilePos& tp, const GfLanePos& l) {
    const int oh = tp.oh0 + l.t, ow = tp.ow0 + l.q * kGfStrip;
    if (!l.active || tp.k0 + l.kb * kGfKB >= g.Cgo || oh >= g.Ho || ow >= g.Wo) return 0;
    return g.Wo - ow < kGfStrip ? g.Wo - ow : kGfStrip;
}
FQ_GEOM_HD unsigned gf_out_off(const GfGeom& g, const GfTilePos& tp, const GfLanePos& l, int kk) {
    const unsigned plane = tp.n * (unsigned)g.K + tp.grp * (unsigned)g.Cgo + (unsigned)(tp.k0 + l.kb * kGfKB + kk);
    return (plane * (unsigned)g.Ho + (unsigned)(tp.oh0 + l.t)) * (unsigned)g.Wo + (unsigned)(tp.ow0 + l.q * kGfStrip);
}

}  // namespace fq
