// fq_deconv_i8_geom.h -- the host guards, the launch geometry and the index arithmetic of the int8 transposed convolution
// (fq_deconv_i8.hip), kept apart from the kernel so that the same functions compile as host code: scripts/deconv_geom_check.cpp
// walks them, lane by lane, over the shapes the GPU tests and the model launch.
//
//   P = (H-1) sh - 2 ph + R + oph,  Q = (W-1) sw - 2 pw + S + opw
//   acc[n][oh][ow][k] = sum x[n][ih][iw][c] w[c][k][r][s]   over c < C and the taps with oh + ph - r = ih sh, ow + pw - s = iw sw
//
// Sub-pixel phases.  Output row oh = fh + sh j (fh < sh its PHASE ROW, j its index on the phase plane) is reached through the
// kernel rows r = a + sh th only, a = (fh + ph) mod sh, th < Th = ceil((R - a) / sh), and then ih = j + dh - th with
// dh = (fh + ph) / sh: a dense stride-1 correlation over x with Th (x Tw) taps.  Th = 0 (a >= R) is a phase without a tap: its
// outputs are tail(0, bias).  The same per column.  A phase plane has at most PJ x QJ = ceil(P / sh) x ceil(Q / sw) pixels; rows
// and columns beyond P, Q (phases that are one shorter) are walked and masked.
//
// Packed weights: phase f = fh sw + fw after phase, each [Kpad][Th Tw][Cpad] (k, tap th Tw + tw, channel; zeros for k >= K and
// c >= C), so that row k of a phase is a run of chunks = Th Tw Cpad / 16 16-byte chunks, the phase's reduction axis.  Every tap
// lies in exactly one phase: Kpad R S Cpad bytes in all.
//
// An ITEM is (pixel tile mt, channel block kb, phase f), item = (mt KB + kb) F + f: 128 phase-plane pixels (32 per wave, one per
// lane of a half-wave) x KW output channels of one phase.  At most kDcMaxBlocks workgroups; a workgroup takes items blockIdx.x,
// + blocks, ...  A lane's pixel m = 128 mt + its slot is split into (n, j, i) by division ONCE (dc_pix_begin); dc_walk_step then
// advances (f, kb, mt) by the stride's digits with two carries and the pixel by the digits of 128 (dmt + carry) pixels.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FQ_DC_HD __host__ __device__ __forceinline__
#else
#define FQ_DC_HD inline
#endif

namespace fq {

constexpr int kDcBlock = 256;             // threads per workgroup: 4 waves x 32 pixels
constexpr int kDcTilePix = 128;
constexpr int kDcMaxBlocks = 2048;        // 256 CUs x 8 workgroups: workgroups stride over the rest of the items
constexpr int kDcMaxPhases = 16;          // stride <= 4 per axis
constexpr int kDcOk = 0, kDcInvalid = -1, kDcUnsupported = -4;      // FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED (include/fq.h)
constexpr unsigned kDcOutOfRange = 0x80000000u;                     // beyond num_records of either buffer descriptor: zeros

FQ_DC_HD int dc_pad16(int c) { return (c + 15) / 16 * 16; }
FQ_DC_HD int dc_ceil_div(int a, int b) { return (a + b - 1) / b; }

// The layers taken (host arithmetic only; what fq_deconv2d_i8_supported answers).  The accumulator bound: a phase sums at most
// ceil(R / sh) ceil(S / sw) C products of magnitude <= 2^14; with the rounding constant and the clamped bias shifted by rs
// (fq_int_tail.h: |qb| <= 255) it must stay inside int32.
FQ_DC_HD bool dc_supported(int C, int K, int groups, int R, int S, int sh, int sw, int ph, int pw, int oph, int opw, int dil_h,
                           int dil_w, int rs_min, int rs_max) {
    if (C < 1 || K < 1 || groups != 1 || dil_h != 1 || dil_w != 1) return false;
    if (R < 1 || R > 8 || S < 1 || S > 8 || sh < 1 || sh > 4 || sw < 1 || sw > 4) return false;
    if (ph < 0 || ph >= R || pw < 0 || pw >= S || oph < 0 || oph >= sh || opw < 0 || opw >= sw) return false;
    if (rs_min < 1 || rs_min > rs_max || rs_max > 16) return false;
    const long taps = (long)dc_ceil_div(R, sh) * dc_ceil_div(S, sw);
    return taps * C * 16384L + 65536L + (255L << rs_max) < 0x7fffffffL;
}

FQ_DC_HD size_t dc_packed_bytes(int C, int K, int R, int S) {
    return (size_t)dc_pad16(K) * (size_t)R * (size_t)S * (size_t)dc_pad16(C);
}

// The entry point's verdict on everything but the launch itself: scalars first, then N == 0, then the pointers (given as
// addresses).  kDcOk with *launch == 0: nothing to do (N == 0).
FQ_DC_HD int dc_guard(uintptr_t x, uintptr_t w, uintptr_t qbias, uintptr_t q, int Cpad, int Kpad, int act_lo, int act_hi, int N, int H,
                      int W, int C, int K, int R, int S, int sh, int sw, int ph, int pw, int oph, int opw, int rs, int ob, int* launch) {
    *launch = 0;
    if (!(-128 <= act_lo && act_lo <= 0 && 0 <= act_hi && act_hi <= 127)) return kDcInvalid;
    if (rs < -120 || rs > 120 || ob < -120 || ob > 120) return kDcInvalid;
    if (N < 0 || H < 1 || W < 1 || C < 1 || K < 1 || R < 1 || S < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || oph < 0 || opw < 0)
        return kDcInvalid;
    if (!dc_supported(C, K, 1, R, S, sh, sw, ph, pw, oph, opw, 1, 1, rs, rs)) return kDcUnsupported;
    if (Cpad != dc_pad16(C) || Kpad != dc_pad16(K)) return kDcInvalid;
    const long P = (long)(H - 1) * sh - 2 * ph + R + oph, Q = (long)(W - 1) * sw - 2 * pw + S + opw;
    if (P < 1 || Q < 1) return kDcInvalid;
    // 32-bit byte offsets into x, the packed weights and q; 32-bit pixel and item counts
    if ((long)N * H >= 0x7fffffffL / W || (long)N * H * W * Cpad >= 0x7fffffffL) return kDcUnsupported;
    if ((long)N * P >= 0x3fffffffL / Q || (long)N * P * Q * Kpad >= 0x3fffffffL) return kDcUnsupported;
    if ((long)Kpad * R * S * Cpad >= 0x7fffffffL) return kDcUnsupported;
    if (N == 0) return kDcOk;
    if (!x || !w || !qbias || !q || ((x | w | q) & 15u) || (qbias & 3u)) return kDcInvalid;
    *launch = 1;
    return kDcOk;
}

struct DcGeom {
    int N, H, W, C, K, R, S, sh, sw, ph, pw, P, Q, Cpad, Kpad;
    int c16;                               // Cpad / 16
    int KW;                                // output channels of an item: 32, or 64 where Kpad > 32
    unsigned PJ, QJ;                       // the largest phase plane
    unsigned M;                            // N PJ QJ: walked pixels of one phase
    unsigned F, KB, MT;                    // phases, channel blocks, pixel tiles
    unsigned items, blocks;
    unsigned df, dkb, dmt;                 // blocks = (dmt KB + dkb) F + df
    unsigned si[2], sj[2], sn[2];          // 128 (dmt + carry) pixels = (sn PJ + sj) QJ + si
    unsigned x_bytes, w_bytes, q_bytes;
};

// (a geometry the guard took, N >= 1)
FQ_DC_HD DcGeom dc_geom(int N, int H, int W, int C, int K, int R, int S, int sh, int sw, int ph, int pw, int oph, int opw) {
    DcGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.K = K; g.R = R; g.S = S; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
    g.P = (H - 1) * sh - 2 * ph + R + oph; g.Q = (W - 1) * sw - 2 * pw + S + opw;
    g.Cpad = dc_pad16(C); g.Kpad = dc_pad16(K); g.c16 = g.Cpad / 16;
    g.KW = g.Kpad > 32 ? 64 : 32;
    g.PJ = (unsigned)dc_ceil_div(g.P, sh); g.QJ = (unsigned)dc_ceil_div(g.Q, sw);
    g.M = (unsigned)N * g.PJ * g.QJ;
    g.F = (unsigned)(sh * sw); g.KB = (unsigned)dc_ceil_div(g.Kpad, g.KW); g.MT = (g.M + kDcTilePix - 1u) / kDcTilePix;
    g.items = g.MT * g.KB * g.F;
    g.blocks = g.items > (unsigned)kDcMaxBlocks ? (unsigned)kDcMaxBlocks : g.items;
    g.df = g.blocks % g.F;
    const unsigned rest = g.blocks / g.F;
    g.dkb = rest % g.KB; g.dmt = rest / g.KB;
    for (unsigned c = 0; c < 2; ++c) {
        const unsigned pix = (g.dmt + c) * kDcTilePix, row = pix / g.QJ;
        g.si[c] = pix % g.QJ; g.sj[c] = row % g.PJ; g.sn[c] = row / g.PJ;
    }
    g.x_bytes = (unsigned)N * (unsigned)H * (unsigned)W * (unsigned)g.Cpad;
    g.w_bytes = (unsigned)dc_packed_bytes(C, K, R, S);
    g.q_bytes = (unsigned)N * (unsigned)g.P * (unsigned)g.Q * (unsigned)g.Kpad;
    return g;
}

// One axis of a phase: first output index f, first kernel index a, taps T, input shift d
struct DcAxis {
    int f, a, T, d;
};
FQ_DC_HD DcAxis dc_axis(int f, int pad, int stride, int ksize) {
    DcAxis x;
    x.f = f; x.a = (f + pad) % stride; x.d = (f + pad) / stride;
    x.T = x.a < ksize ? (ksize - x.a + stride - 1) / stride : 0;
    return x;
}

struct DcPhase {
    DcAxis h, w;
    int chunks;                            // Th Tw c16: 16-byte chunks of the reduction axis
    unsigned woff;                         // byte offset of the phase's [Kpad][chunks][16] block in the packed weights
};
FQ_DC_HD DcPhase dc_phase(const DcGeom& g, unsigned f) {
    DcPhase p;
    const int fh = (int)f / g.sw, fw = (int)f % g.sw;
    p.h = dc_axis(fh, g.ph, g.sh, g.R); p.w = dc_axis(fw, g.pw, g.sw, g.S);
    p.chunks = p.h.T * p.w.T * g.c16;
    // taps of the phases in front: whole phase rows, then the phases of this row
    int taps = 0;
    for (int e = 0; e < fh; ++e) taps += dc_axis(e, g.ph, g.sh, g.R).T * g.S;
    for (int e = 0; e < fw; ++e) taps += p.h.T * dc_axis(e, g.pw, g.sw, g.S).T;
    p.woff = (unsigned)taps * (unsigned)g.Kpad * (unsigned)g.Cpad;
    return p;
}

// item = (mt KB + kb) F + f; the lane's pixel m = 128 mt + slot = (n PJ + j) QJ + i
struct DcWalk {
    unsigned f, kb, mt;
    unsigned n, j, i;
};
FQ_DC_HD DcWalk dc_walk_begin(const DcGeom& g, unsigned item, unsigned slot) {
    DcWalk s;
    const unsigned rest = item / g.F;
    s.f = item - rest * g.F;
    s.mt = rest / g.KB;
    s.kb = rest - s.mt * g.KB;
    const unsigned m = s.mt * kDcTilePix + slot, row = m / g.QJ;
    s.i = m - row * g.QJ;
    s.n = row / g.PJ;
    s.j = row - s.n * g.PJ;
    return s;
}
FQ_DC_HD void dc_walk_step(const DcGeom& g, DcWalk& s) {
    s.f += g.df;
    if (s.f >= g.F) { s.f -= g.F; ++s.kb; }
    s.kb += g.dkb;
    unsigned c = 0;
    if (s.kb >= g.KB) { s.kb -= g.KB; c = 1; }
    s.mt += g.dmt + c;
    s.i += g.si[c];
    if (s.i >= g.QJ) { s.i -= g.QJ; ++s.j; }
    s.j += g.sj[c];
    if (s.j >= g.PJ) { s.j -= g.PJ; ++s.n; }
    s.n += g.sn[c];
}

// does the lane's pixel exist in this phase?  (n >= N: past the last tile's pixels; oh, ow: the shorter phases)
FQ_DC_HD bool dc_pix_ok(const DcGeom& g, const DcPhase& p, const DcWalk& s) {
    return s.n < (unsigned)g.N && p.h.f + g.sh * (int)s.j < g.P && p.w.f + g.sw * (int)s.i < g.Q;
}

// The reduction axis of a phase, chunk by chunk: chunk ch = (th Tw + tw) c16 + cc.  (advanced by increments, not divided)
struct DcChunk {
    int ch, th, tw, cc;
};
FQ_DC_HD DcChunk dc_chunk_begin() { return DcChunk{0, 0, 0, 0}; }
FQ_DC_HD void dc_chunk_next(const DcGeom& g, const DcPhase& p, DcChunk& c) {
    ++c.ch;
    if (++c.cc == g.c16) {
        c.cc = 0;
        if (++c.tw == p.w.T) { c.tw = 0; ++c.th; }
    }
}

// byte offset in x of the lane's 16 input channels for chunk c, or kDcOutOfRange (zeros): no such pixel, a tap outside the image,
// a chunk past the end of the axis
FQ_DC_HD unsigned dc_x_off(const DcGeom& g, const DcPhase& p, const DcWalk& s, bool pix_ok, const DcChunk& c) {
    const int ih = (int)s.j + p.h.d - c.th, iw = (int)s.i + p.w.d - c.tw;
    const bool ok = pix_ok && c.ch < p.chunks && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
    return ok ? ((s.n * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw) * (unsigned)g.Cpad + 16u * (unsigned)c.cc : kDcOutOfRange;
}
// byte offset in the packed weights of chunk ch of output channel k, or kDcOutOfRange
FQ_DC_HD unsigned dc_w_off(const DcGeom& g, const DcPhase& p, int k, int ch) {
    return (k < g.Kpad && ch < p.chunks) ? p.woff + ((unsigned)k * (unsigned)p.chunks + (unsigned)ch) * 16u : kDcOutOfRange;
}
// byte offset in q of channel k of the lane's output pixel (dc_pix_ok)
FQ_DC_HD unsigned dc_q_off(const DcGeom& g, const DcPhase& p, const DcWalk& s, int k) {
    const unsigned oh = (unsigned)p.h.f + (unsigned)g.sh * s.j, ow = (unsigned)p.w.f + (unsigned)g.sw * s.i;
    return ((s.n * (unsigned)g.P + oh) * (unsigned)g.Q + ow) * (unsigned)g.Kpad + (unsigned)k;
}

// Accumulator layout of v_mfma_i32_32x32x32_i8 with the weights as A and the pixels as B: register e of half-wave `half` is output
// channel (e & 3) + 8 (e >> 2) + 4 half of the 32, the lane's own pixel.  Registers 4 g .. 4 g + 3 are four consecutive channels.
FQ_DC_HD int dc_acc_channel(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

}  // namespace fq
