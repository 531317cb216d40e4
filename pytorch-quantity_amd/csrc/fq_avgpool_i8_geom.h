// fq_avgpool_i8_geom.h -- the lane -> (output chunk, window taps, divisor, addresses) arithmetic of the windowed int8 NHWC
// average pooling (fq_avgpool_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/avgpool_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every load lies inside the source,
// that the taps of an output are exactly window ∩ image, that the divisor is the rule's and that every output chunk is written
// exactly once.
//
// The source is [N][H][W][Cpad] bytes, the output [N][P][Q][Cpad]; a CHUNK is 16 consecutive channels of one pixel (one dwordx4),
// CH = Cpad / 16 chunks per pixel.  Output chunk i = ((n P + p) Q + q) CH + k: channel fastest, so a wave stores whole contiguous
// pixels.  A tap outside the image is SKIPPED (never clamped onto the border as the max-pool may: that would count a pixel twice),
// so the window is cut to [h0, h1) x [w0, w1) once per output pixel and the loops run over real pixels only.
#pragma once

#if defined(__HIPCC__)
#define FQ_AVG_HD __host__ __device__ __forceinline__
#else
#define FQ_AVG_HD inline
#endif

namespace fq {

constexpr int kAvgBlock = 256;         // threads per workgroup
constexpr int kAvgMaxBlocks = 2048;    // 256 CUs x 8 workgroups: the lanes walk the rest of the chunks by the grid size
constexpr int kAvgMaxTaps = 64;        // |S| <= 64 * 128 = 8192: a lane accumulates in packed int16
constexpr int kAvgMaxShift = 8;

struct AvgGeom {
    int N, H, W;                       // source plane
    int C, Cpad, CH;                   // real / stored channels, CH = Cpad / 16
    int P, Q;                          // output plane (floor mode)
    int kh, kw, sh, sw, ph, pw;
    int cip;                           // count_include_pad
    unsigned nchunks;                  // N * P * Q * CH  (< 2^27: the output is below 2^31 - 1 bytes)
};

// floor-mode output size, or 0 when the padded image is smaller than the window
FQ_AVG_HD int avg_out_size(int in, int k, int s, int p) { return in + 2 * p - k < 0 ? 0 : (in + 2 * p - k) / s + 1; }

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

// byte offset of the 16-byte tap (n, ih, iw, chunk k) in the source; below 2^31 - 1 (the entry point bounds the source)
FQ_AVG_HD unsigned avg_tap_offset(const AvgGeom& g, int n, int ih, int iw, int k) {
    return (((unsigned)n * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw) * (unsigned)g.Cpad + 16u * (unsigned)k;
}

// byte mask of dword t of chunk k: 0xff for the channels below C
FQ_AVG_HD unsigned avg_dword_mask(const AvgGeom& g, int k, int t) {
    int h = g.C - 16 * k - 4 * t;                           // real channels in this dword and the ones behind it
    h = h < 0 ? 0 : (h > 4 ? 4 : h);
    return h == 4 ? 0xffffffffu : (1u << (8 * h)) - 1u;
}

FQ_AVG_HD long avg_blocks(const AvgGeom& g) {
    long b = ((long)g.nchunks + kAvgBlock - 1) / kAvgBlock;
    return b > kAvgMaxBlocks ? kAvgMaxBlocks : b;
}

}  // namespace fq
