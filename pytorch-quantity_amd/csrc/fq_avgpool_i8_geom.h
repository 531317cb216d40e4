// fq_avgpool_i8_geom.h -- the lane -> (output item, window taps, divisor, byte offsets, channel mask) arithmetic of the windowed
// NHWC average pooling over an int8 activation or an int16 NewAdd sum (fq_avgpool_i8.hip), kept apart from the kernel so that the
// same functions compile as host code: scripts/avgpool_geom_check.cpp walks them over the shapes the GPU tests run and asserts that
// every load lies inside the source, that the taps of an output are exactly window ∩ image, that the divisor is the rule's and that
// every output byte is written exactly once.
//
// The source is [N][H][W][Cpad] elements of Src::kBytes bytes, the output [N][P][Q][Cpad] int8.  An ITEM (a CHUNK where the source
// is int8) is the Src::kLane consecutive channels of one output pixel that one lane owns: 16 source bytes per tap -- one dwordx4
// load for either source --, Src::kOutBytes output bytes.  CH = Cpad / Src::kLane items per pixel; item i = ((n P + p) Q + q) CH + k:
// channel fastest, so a wave loads and stores whole contiguous pixels.  A tap outside the image is SKIPPED (never clamped onto the
// border as the max-pool may: that would count a pixel twice), so the window is cut to [h0, h1) x [w0, w1) once per output pixel
// and the loops run over real pixels only.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define FQ_AVG_HD __host__ __device__ __forceinline__
#else
#define FQ_AVG_HD inline
#endif

namespace fq {

constexpr int kAvgBlock = 256;         // threads per workgroup
constexpr int kAvgMaxBlocks = 2048;    // 256 CUs x 8 workgroups: the lanes walk the rest of the items by the grid size
constexpr int kAvgMaxTaps = 64;        // |S| <= 64 * 128 = 8192 (int8: packed int16 holds it), 64 * 32768 = 2^21 (int16: int32)
constexpr int kAvgMaxShift = 8;

// The two sources.  Compile-time constants, so the offsets below stay shifts.
struct AvgSrcI8 {
    static constexpr int kBytes = 1;       // per source element
    static constexpr int kLane = 16;       // channels per lane
    static constexpr int kOutBytes = 16;   // per item: one dwordx4 store
};
struct AvgSrcI16 {
    static constexpr int kBytes = 2;
    static constexpr int kLane = 8;
    static constexpr int kOutBytes = 8;    // one dwordx2 store
};

struct AvgGeom {
    int N, H, W;                       // source plane
    int C, Cpad, CH;                   // real / stored channels, CH = Cpad / Src::kLane
    int P, Q;                          // output plane (floor mode)
    int kh, kw, sh, sw, ph, pw;
    int cip;                           // count_include_pad
    unsigned nchunks;                  // N * P * Q * CH  (< 2^28: the output is below 2^31 - 1 bytes)
};

// floor-mode output size, or 0 when the padded image is smaller than the window
FQ_AVG_HD int avg_out_size(int in, int k, int s, int p) { return in + 2 * p - k < 0 ? 0 : (in + 2 * p - k) / s + 1; }

// The one builder of an AvgGeom, for arguments the entry point admits (Cpad % 16 == 0, both tensors below 2^31 - 1 bytes)
template <class Src>
FQ_AVG_HD AvgGeom avg_geom(int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw, int ph, int pw, int cip) {
    AvgGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.Cpad = Cpad; g.CH = Cpad / Src::kLane;
    g.P = avg_out_size(H, kh, sh, ph); g.Q = avg_out_size(W, kw, sw, pw);
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
    g.cip = cip ? 1 : 0;
    g.nchunks = (unsigned)((long)N * g.P * g.Q * g.CH);
    return g;
}

struct AvgChunk { int n, p, q, k; };

FQ_AVG_HD AvgChunk avg_chunk(const AvgGeom& g, unsigned i) {
    AvgChunk c;
    c.k = (int)(i % (unsigned)g.CH);
    unsigned r = i / (unsigned)g.CH;
    c.q = (int)(r % (unsigned)g.Q);
    r /= (unsigned)g.Q;
    c.p = (int)(r % (unsigned)g.P);
    c.n = (int)(r / (unsigned)g.P);
    return c;
}

// window ∩ image of output pixel (p, q): rows [h0, h1), columns [w0, w1); never empty (2 pad <= kernel, floor mode)
struct AvgWindow { int h0, h1, w0, w1; };

FQ_AVG_HD AvgWindow avg_window(const AvgGeom& g, int p, int q) {
    AvgWindow w;
    const int hs = p * g.sh - g.ph, ws = q * g.sw - g.pw;
    w.h0 = hs < 0 ? 0 : hs;
    w.h1 = hs + g.kh < g.H ? hs + g.kh : g.H;
    w.w0 = ws < 0 ? 0 : ws;
    w.w1 = ws + g.kw < g.W ? ws + g.kw : g.W;
    return w;
}

// torch's divisor: the whole (padded, never cut in floor mode) window with count_include_pad, else the taps inside the image
FQ_AVG_HD int avg_divisor(const AvgGeom& g, const AvgWindow& w) { return g.cip ? g.kh * g.kw : (w.h1 - w.h0) * (w.w1 - w.w0); }

// bytes between two taps of one window row: one source pixel
template <class Src>
FQ_AVG_HD unsigned avg_tap_step(const AvgGeom& g) { return (unsigned)Src::kBytes * (unsigned)g.Cpad; }

// byte offset of the 16-byte tap (n, ih, iw, item k) in the source; below 2^31 - 1 (the entry point bounds the source's bytes)
template <class Src>
FQ_AVG_HD unsigned avg_tap_offset(const AvgGeom& g, int n, int ih, int iw, int k) {
    return (((unsigned)n * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw) * avg_tap_step<Src>(g) + 16u * (unsigned)k;
}

// byte offset of item i in the output
template <class Src>
FQ_AVG_HD size_t avg_store_offset(unsigned i) { return (size_t)i * Src::kOutBytes; }

// byte mask of output dword t of item k: 0xff for the channels below C
template <class Src>
FQ_AVG_HD unsigned avg_dword_mask(const AvgGeom& g, int k, int t) {
    int h = g.C - Src::kLane * k - 4 * t;                   // real channels in this dword and the ones behind it
    h = h < 0 ? 0 : (h > 4 ? 4 : h);
    return h == 4 ? 0xffffffffu : (1u << (8 * h)) - 1u;
}

FQ_AVG_HD long avg_blocks(const AvgGeom& g) {
    long b = ((long)g.nchunks + kAvgBlock - 1) / kAvgBlock;
    return b > kAvgMaxBlocks ? kAvgMaxBlocks : b;
}

}  // namespace fq
