// fq_dwconv_dil_i8_geom.h -- the tile / lane -> address arithmetic of the atrous depthwise int8 convolution
// (fq_dwconv_dil_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/dwconv_dil_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every address a lane may
// touch lies inside its tensor and every output dword is written once.
//
// The lattice walk.  A stride-1 convolution with dilation d reads, for output pixel (p, q), the input pixels
// (p - pad_h + r*d, q - pad_w + s*d).  With p = fh + d*pp and q = fw + d*qq (fh = p mod d, fw = q mod d: the PHASE) that is
// ((fh - pad_h) + d*(pp + r), (fw - pad_w) + d*(qq + s)): on the lattice of step d through (fh - pad_h, fw - pad_w) the taps of
// one kernel row are consecutive lattice pixels, and the d*d phases are independent dense stride-1 convolutions.  A tile is
// TP x 4 outputs of ONE phase; the address functions of the dense kernel (fq_dwconv_i8_geom.h) serve unchanged, a lattice
// pixel being an image pixel at a step of d.
#pragma once
#include "fq_dwconv_i8_geom.h"

namespace fq {

constexpr int kDwDilMin = 2, kDwDilMax = 64;       // dilation 1 is the dense kernel's

struct DwDilGeom {
    DwGeom g;                          // the planes; g.PB x g.QB: bands x blocks of the LARGEST phase sub-plane (phase 0)
    int d;                             // dilation, both axes
    int dh, dw;                        // phases that own an output row / column: min(d, P), min(d, Q)
};                                     // g.tiles = N * PB * dh * QB * dw

// the sub-plane of phase f along an axis of n outputs: ceil((n - f) / d) lattice positions (f < min(d, n): at least one)
FQ_DW_HD int dwd_phase_len(int n, int f, int d) { return (n - f + d - 1) / d; }

// Tile number -> (image, row band, row phase, column block, column phase), the column phase FASTEST: neighbouring tiles are
// neighbouring pixels, so for C4 < 64 a wave's loads and stores cover contiguous bytes, and the d phases of one line touch
// the same cache lines close in time.  The digits are a mixed-radix number; n, the last, is unbounded.
struct DwDilPos { int n, pb, fh, qb, fw; };
FQ_DW_HD DwDilPos dwd_decode(const DwDilGeom& a, unsigned tile) {
    DwDilPos t;
    t.fw = (int)(tile % (unsigned)a.dw); tile /= (unsigned)a.dw;
    t.qb = (int)(tile % (unsigned)a.g.QB); tile /= (unsigned)a.g.QB;
    t.fh = (int)(tile % (unsigned)a.dh); tile /= (unsigned)a.dh;
    t.pb = (int)(tile % (unsigned)a.g.PB);
    t.n = (int)(tile / (unsigned)a.g.PB);
    return t;
}
// pos += step, digit by digit with carry (each digit of both is below its radix, so one subtraction per digit): the lanes
// decode their first tile and their stride once and then walk without a division, whatever d is
FQ_DW_HD void dwd_advance(const DwDilGeom& a, DwDilPos& t, const DwDilPos& step) {
    int c;
    t.fw += step.fw; c = t.fw >= a.dw; t.fw -= c ? a.dw : 0;
    t.qb += step.qb + c; c = t.qb >= a.g.QB; t.qb -= c ? a.g.QB : 0;
    t.fh += step.fh + c; c = t.fh >= a.dh; t.fh -= c ? a.dh : 0;
    t.pb += step.pb + c; c = t.pb >= a.g.PB; t.pb -= c ? a.g.PB : 0;
    t.n += step.n + c;
}
// the tile's first output pixel (rows p0 + d*t, columns q0 + d*j) and first lattice pixel (rows ih0 + d*i, columns iw0 + d*k)
struct DwDilTile { int p0, q0, ih0, iw0; };
template <int TP>
FQ_DW_HD DwDilTile dwd_tile(const DwDilGeom& a, const DwDilPos& t) {
    DwDilTile o;
    o.p0 = t.fh + a.d * (t.pb * TP);
    o.q0 = t.fw + a.d * (t.qb * kDwTQ);
    o.ih0 = o.p0 - a.g.pad_h;
    o.iw0 = o.q0 - a.g.pad_w;
    return o;
}

// The geometry of a launch, or false where the 32-bit tile arithmetic would not hold it (host only; the caller has checked
// the shape: stride 1, 2 <= d <= 64, pads within the span, P, Q >= 1).
inline bool dwd_make(DwDilGeom& a, int TP, int N, int H, int W, int Cpad, int R, int d, int pad_h, int pad_w) {
    DwGeom& g = a.g;
    g.N = N; g.H = H; g.W = W; g.Cpad = Cpad; g.C4 = Cpad / 4; g.pad_h = pad_h; g.pad_w = pad_w;
    g.P = H + 2 * pad_h - d * (R - 1);
    g.Q = W + 2 * pad_w - d * (R - 1);
    a.d = d;
    a.dh = d < g.P ? d : g.P;
    a.dw = d < g.Q ? d : g.Q;
    g.PB = (dwd_phase_len(g.P, 0, d) + TP - 1) / TP;
    g.QB = (dwd_phase_len(g.Q, 0, d) + kDwTQ - 1) / kDwTQ;
    const long tiles = (long)N * g.PB * a.dh * g.QB * a.dw;
    g.tiles = (unsigned)tiles;
    // a lane's tile counter goes up to tiles + its stride (at most kDwMaxBlocks * kDwBlock), lanes = tiles * C4
    return tiles > 0 && tiles * g.C4 < 0x7fffffffL;
}
inline unsigned dwd_blocks(const DwDilGeom& a) {
    long blocks = ((long)a.g.tiles * a.g.C4 + kDwBlock - 1) / kDwBlock;
    return (unsigned)(blocks > kDwMaxBlocks ? kDwMaxBlocks : blocks);
}

}  // namespace fq
