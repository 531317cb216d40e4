// fq_avgpool_i16_geom.h -- the lane -> (output item, window taps, divisor, byte offsets, channel mask) arithmetic of the windowed
// average pooling over an int16 NHWC sum (fq_avgpool_i16.hip), kept apart from the kernel so that the same functions compile as
// host code: scripts/avgpool_i16_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every load lies
// inside the source, that the taps of an output are exactly window ∩ image, that the divisor is the rule's and that every output
// byte is written exactly once.
//
// The source is [N][H][W][Cpad] int16 (2 Cpad bytes per pixel), the output [N][P][Q][Cpad] int8.  An ITEM is 8 consecutive
// channels of one output pixel: one 16-byte load per tap, one 8-byte store.  CH = Cpad / 8 items per pixel (even: Cpad % 16 == 0);
// item i = ((n P + p) Q + q) CH + k, channel fastest, so a wave loads 1 KiB and stores 512 contiguous bytes.  The window cut, the
// divisor and the floor-mode output size are the int8 pool's own functions (fq_avgpool_i8_geom.h: avg_out_size, avg_window,
// avg_divisor, avg_chunk with this CH); only what depends on the element size and on the item's width is new here.
#pragma once

#include <cstddef>

#include "fq_avgpool_i8_geom.h"

namespace fq {

constexpr int kAvg16Lane = 8;          // channels per lane: 16 source bytes, 8 output bytes

// An AvgGeom for the int16 source: CH counts items of 8 channels, nchunks = N P Q CH  (< 2^28: the output is below 2^31 - 1 bytes)
FQ_AVG_HD AvgGeom avg16_geom(int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw, int ph, int pw, int cip) {
    AvgGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.Cpad = Cpad; g.CH = Cpad / kAvg16Lane;
    g.P = avg_out_size(H, kh, sh, ph); g.Q = avg_out_size(W, kw, sw, pw);
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
    g.cip = cip ? 1 : 0;
    g.nchunks = (unsigned)((long)N * g.P * g.Q * g.CH);
    return g;
}

// byte offset of the 16-byte tap (n, ih, iw, item k) in the source; below 2^31 - 1 (the entry point bounds the source's bytes)
FQ_AVG_HD unsigned avg16_tap_offset(const AvgGeom& g, int n, int ih, int iw, int k) {
    return (((unsigned)n * (unsigned)g.H + (unsigned)ih) * (unsigned)g.W + (unsigned)iw) * (2u * (unsigned)g.Cpad) + 16u * (unsigned)k;
}

// bytes between two taps of one window row
FQ_AVG_HD unsigned avg16_tap_step(const AvgGeom& g) { return 2u * (unsigned)g.Cpad; }

// byte offset of item i in the output
FQ_AVG_HD size_t avg16_store_offset(unsigned i) { return (size_t)i * kAvg16Lane; }

// byte mask of output dword t (0, 1) of item k: 0xff for the channels below C
FQ_AVG_HD unsigned avg16_dword_mask(const AvgGeom& g, int k, int t) {
    int h = g.C - kAvg16Lane * k - 4 * t;                   // real channels in this dword and the ones behind it
    h = h < 0 ? 0 : (h > 4 ? 4 : h);
    return h == 4 ? 0xffffffffu : (1u << (8 * h)) - 1u;
}

}  // namespace fq
