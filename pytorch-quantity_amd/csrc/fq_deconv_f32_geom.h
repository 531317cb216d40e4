// fq_deconv_f32_geom.h -- the launch plan and the work-item / lane -> address arithmetic of the transposed fp32 convolution
// (fq_deconv_f32.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/deconv_f32_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every load lies inside x
// or wt, every store inside y, and every output element is written exactly once.
//
// Sub-pixel phases.  Output row oh = rp + stride * ohq belongs to ROW PHASE rp (0 .. stride-1): only the kernel rows
// r = (rp + pad) mod stride, + stride, ... reach it, from input row ih = ohq + (rp + pad - r) / stride (an exact quotient,
// negative or past the plane for a tap outside the image).  Output column ow = cp + stride * q belongs to COLUMN PHASE cp in
// the same way: s = (cp + pad) mod stride, + stride, ..., iw = q + (cp + pad - s) / stride.  On the sub-grid of one (rp, cp) the
// layer is a dense stride-1 correlation of x over those taps: a GEMM with M = Cout, K = (taps, Cin) and the flat list of
// sub-grid pixels as columns.
//
// A work item is one (row phase, tile of 32 MW output channels, tile of 32 NW columns); a column is j = (n * Hq + ohq) * Qmax + q
// with Hq = rows of the row phase and Qmax = ceil(Wo / stride), so small planes cost no padding between rows or images.  The
// four waves of a workgroup sit MW x NW; a wave owns 32 channels x 32 columns x ALL stride column phases of those columns
// (stride accumulator tiles): lane (column q) then holds the `stride` neighbouring floats ow = stride q .. stride q + stride - 1
// of an output row and stores them as one contiguous run.
#pragma once
#include "fq_f32_geom_common.h"

namespace fq {

constexpr int kDcBlock = 256;              // threads per workgroup: 4 waves
constexpr int kDcMaxStride = 4;
constexpr int kDcMaxKernel = 8;
constexpr int kDcMaxBlocks = 2048;         // 256 CUs x 8 workgroups: the workgroups walk the rest of the work items
constexpr int kDcMaxBlocksHist = 1024;     // the histogram form flushes 2048 bins per workgroup: a smaller persistent grid

struct DcGeom {
    int N, Cin, Hin, Win, Cout, R, S, stride, pad, Ho, Wo;
    int Qmax;                              // ceil(Wo / stride): columns of a sub-grid row (the last ones exist for some cp only)
    int MW, NW;                            // waves along the channels / the columns (MW * NW = 4)
    int tiles_m;                           // ceil(Cout / (32 MW))
    int Hq[kDcMaxStride];                  // output rows of row phase rp
    unsigned cols[kDcMaxStride];           // N * Hq[rp] * Qmax
    unsigned item0[kDcMaxStride + 1];      // first work item of row phase rp; item0[stride] = items
    unsigned items;
    unsigned plane_in;                     // Hin * Win
};

inline bool dc_supported(int Cin, int Cout, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int outpad_h,
                         int outpad_w, int dil_h, int dil_w, int H, int W) {
    if (groups != 1 || dil_h != 1 || dil_w != 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return false;
    if (R < 1 || S < 1 || R > kDcMaxKernel || S > kDcMaxKernel) return false;
    if (stride_h != stride_w || stride_h < 1 || stride_h > kDcMaxStride) return false;
    if (pad_h != pad_w || pad_h < 0 || pad_h >= (R < S ? R : S)) return false;
    if (outpad_h != outpad_w || outpad_h < 0 || outpad_h >= stride_h) return false;
    if (Cin % 16 != 0 || Cout % 4 != 0) return false;
    const long Ho = (long)(H - 1) * stride_h - 2L * pad_h + R + outpad_h, Wo = (long)(W - 1) * stride_w - 2L * pad_w + S + outpad_w;
    return Ho >= 1 && Wo >= 1;
}

// The plan: a function of the layer's shape alone (never of the statistic that rides on the launch).  The caller has checked
// dc_supported and that x, y and wt stay below 2^30 elements (32-bit element offsets).
inline bool dc_plan(DcGeom& g, int N, int Cin, int Hin, int Win, int Cout, int R, int S, int stride, int pad, int outpad) {
    if (N < 1 || !dc_supported(Cin, Cout, 1, R, S, stride, stride, pad, pad, outpad, outpad, 1, 1, Hin, Win)) return false;
    g.N = N; g.Cin = Cin; g.Hin = Hin; g.Win = Win; g.Cout = Cout; g.R = R; g.S = S; g.stride = stride; g.pad = pad;
    g.Ho = (Hin - 1) * stride - 2 * pad + R + outpad;
    g.Wo = (Win - 1) * stride - 2 * pad + S + outpad;
    g.Qmax = (g.Wo + stride - 1) / stride;
    g.MW = Cout <= 32 ? 1 : (Cout <= 64 ? 2 : 4);
    g.NW = 4 / g.MW;
    g.tiles_m = (Cout + 32 * g.MW - 1) / (32 * g.MW);
    g.plane_in = (unsigned)Hin * (unsigned)Win;
    unsigned at = 0;
    for (int rp = 0; rp < kDcMaxStride; ++rp) {
        g.Hq[rp] = rp < stride && g.Ho > rp ? (g.Ho - rp + stride - 1) / stride : 0;
        g.cols[rp] = (unsigned)N * (unsigned)g.Hq[rp] * (unsigned)g.Qmax;           // <= N * Ho * Wo < 2^30
        g.item0[rp] = at;
        at += (unsigned)g.tiles_m * ((g.cols[rp] + 32u * (unsigned)g.NW - 1u) / (32u * (unsigned)g.NW));
    }
    g.item0[kDcMaxStride] = at;
    g.items = at;
    return at >= 1;
}

inline unsigned dc_grid(const DcGeom& g, bool hist) {
    const unsigned cap = hist ? (unsigned)kDcMaxBlocksHist : (unsigned)kDcMaxBlocks;
    return g.items < cap ? g.items : cap;
}

// work item -> row phase, first output channel and first column of the workgroup's tile (channel tile fastest: the workgroups
// that read the same columns of x run next to each other)
struct DcItemPos { int rp; unsigned m0, j0; };
FQ_GEOM_HD DcItemPos dc_item_pos(const DcGeom& g, unsigned item) {
    DcItemPos p;
    p.rp = 0;
    for (int i = 1; i < kDcMaxStride; ++i)
        if (item >= g.item0[i]) p.rp = i;                        // (an empty row phase has item0[i] == item0[i + 1]: the last one wins)
    const unsigned local = item - g.item0[p.rp];
    const unsigned nt = local / (unsigned)g.tiles_m, mt = local - nt * (unsigned)g.tiles_m;
    p.m0 = mt * 32u * (unsigned)g.MW;
    p.j0 = nt * 32u * (unsigned)g.NW;
    return p;
}

// wave of the workgroup -> its 32 channels and 32 columns inside the workgroup's tile
FQ_GEOM_HD unsigned dc_wave_m(const DcGeom& g, unsigned wave) { return 32u * (wave % (unsigned)g.MW); }
FQ_GEOM_HD unsigned dc_wave_j(const DcGeom& g, unsigned wave) { return 32u * (wave / (unsigned)g.MW); }

// column j of row phase rp -> image, sub-grid row, sub-grid column; valid: the column exists
struct DcColPos { unsigned n; int ohq, q; bool valid; };
FQ_GEOM_HD DcColPos dc_col_pos(const DcGeom& g, int rp, unsigned j) {
    DcColPos c;
    c.valid = j < g.cols[rp];
    const unsigned jj = c.valid ? j : 0u;
    const unsigned t = jj / (unsigned)g.Qmax;
    c.q = (int)(jj - t * (unsigned)g.Qmax);
    const unsigned hq = g.Hq[rp] > 0 ? (unsigned)g.Hq[rp] : 1u;
    c.n = t / hq;
    c.ohq = (int)(t - c.n * hq);
    return c;
}

// first kernel row (column) that reaches phase p: (p + pad) mod stride; the others follow in steps of stride
FQ_GEOM_HD int dc_first_tap(const DcGeom& g, int p) { return (p + g.pad) % g.stride; }

// The source pixel of tap (r, s) for column c of (rp, cp): whether it lies inside the image ("outside: the operand +0.0f",
// also for a column that does not exist); *off is then the element offset of input channel 0 (channel c adds c * plane_in).
FQ_GEOM_HD bool dc_tap_src(const DcGeom& g, const DcColPos& c, int rp, int cp, int r, int s, unsigned* off) {
    const int ih = c.ohq + (rp + g.pad - r) / g.stride;          // exact: r = (rp + pad) mod stride + i * stride
    const int iw = c.q + (cp + g.pad - s) / g.stride;
    const bool ok = c.valid && (unsigned)ih < (unsigned)g.Hin && (unsigned)iw < (unsigned)g.Win;
    *off = ok ? ((c.n * (unsigned)g.Cin) * (unsigned)g.Hin + (unsigned)ih) * (unsigned)g.Win + (unsigned)iw : 0u;
    return ok;
}

// element offset into wt [(r*S + s)*Cin + c][Cout] of (tap, input channel c, output channel k)
FQ_GEOM_HD unsigned dc_w_off(const DcGeom& g, int r, int s, unsigned c, unsigned k) {
    return ((unsigned)(r * g.S + s) * (unsigned)g.Cin + c) * (unsigned)g.Cout + k;
}

// how many of the `stride` neighbouring output columns ow = stride q + cp of column c exist (0: none)
FQ_GEOM_HD int dc_out_count(const DcGeom& g, const DcColPos& c) {
    if (!c.valid) return 0;
    const int left = g.Wo - c.q * g.stride;
    return left < g.stride ? (left > 0 ? left : 0) : g.stride;
}
// element offset into y of output channel k, column phase 0 of column c (column phase cp adds cp)
FQ_GEOM_HD unsigned dc_out_off(const DcGeom& g, const DcColPos& c, int rp, unsigned k) {
    return ((c.n * (unsigned)g.Cout + k) * (unsigned)g.Ho + (unsigned)(rp + c.ohq * g.stride)) * (unsigned)g.Wo +
           (unsigned)(c.q * g.stride);
}

// the output channel of accumulator register e (0 .. 15) in the half-wave h of a 32 x 32 MFMA tile: the four rows of a register
// quad are consecutive
FQ_GEOM_HD unsigned dc_acc_row(int e, unsigned h) { return (unsigned)((e & 3) + 8 * (e >> 2)) + 4u * h; }

}  // namespace fq
