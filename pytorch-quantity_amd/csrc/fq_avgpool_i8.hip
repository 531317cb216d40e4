// fq_avgpool_i8.hip -- windowed nn.AvgPool2d on a resident int8 NHWC activation, re-quantised for the convolution behind it
// (include/fq.h: fq_avgpool_i8_nhwc).
//
// The reference's chain is DeQuantity(g) -> nn.AvgPool2d -> optional nn.ReLU -> Quantity(b) of the consumer.  The source is int8
// on the grid g, so every partial sum of torch's fp32 accumulation is exact and the chain is, per output element and channel,
//   S = sum of x over window ∩ image (int), D = kh kw (count_include_pad) or the number of taps inside the image,
//   f = (float)S / (float)D           ONE correctly rounded fp32 division
//   t = f * 2^(b - g)                 exact
//   y = clamp(relu ? max(rint(t), 0) : rint(t), -128, 127)          rint: half to even
// -- two roundings on purpose (f to fp32, then t to an integer): rounding the rational S 2^shift / D once is another function.
// A bandwidth kernel without LDS:
//   * one lane owns one 16-byte chunk of the output (fq_avgpool_i8_geom.h), channel fastest, so a wave loads and stores whole
//     contiguous pixels; at most 2048 workgroups, every lane steps through the chunks by the grid size;
//   * one dwordx4 load per tap; the window is cut to the image once per output pixel, so a tap outside it is skipped;
//   * bytes are sign-extended two at a time into packed int16 lanes (even bytes: shift up by 8, then a packed arithmetic shift
//     down; odd bytes: the packed shift alone) and accumulated with packed adds: |S| <= 64 * 128 = 8192 (kAvgMaxTaps);
//   * sixteen plain `/` divisions per chunk (the build has -fhip-fp32-correctly-rounded-divide-sqrt and no fast-math), the
//     exact power of two, rintf, ReLU and clamp folded into one fmaxf / fminf pair; channels at and above C are masked to zero
//     whatever the source's padding channels hold; one dwordx4 store.
// Every load is 16-byte aligned and lies inside [x, x + N H W Cpad); scripts/avgpool_geom_check.cpp walks the same functions on
// the host over the tests' shapes.
#include "fq_common.h"
#include "fq_avgpool_i8_geom.h"

namespace fq {

struct AvgParams {
    AvgGeom g;
    float scale;                       // 2^shift
    float lo;                          // 0 with the fused ReLU, else -128
};

typedef unsigned avg_v4u __attribute__((ext_vector_type(4)));
typedef short avg_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned avg_requant(int s, float d, float scale, float lo) {
    const float r = rintf(((float)s / d) * scale);
    return (unsigned)(int)fminf(fmaxf(r, lo), 127.0f) & 0xffu;
}

__global__ __launch_bounds__(kAvgBlock) void avgpool_i8_nhwc_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y, const AvgParams p) {
    const AvgGeom& g = p.g;
    const unsigned stride = gridDim.x * kAvgBlock;
    for (unsigned i = blockIdx.x * kAvgBlock + threadIdx.x; i < g.nchunks; i += stride) {
        const AvgChunk c = avg_chunk(g, i);
        const AvgWindow w = avg_window(g, c.p, c.q);
        avg_s2 ev[4], od[4];                              // running sums of bytes 0, 2 / 1, 3 of each dword
#pragma unroll
        for (int t = 0; t < 4; ++t) ev[t] = od[t] = avg_s2{0, 0};
        for (int ih = w.h0; ih < w.h1; ++ih) {
            unsigned off = avg_tap_offset(g, c.n, ih, w.w0, c.k);
            for (int iw = w.w0; iw < w.w1; ++iw, off += (unsigned)g.Cpad) {
                const avg_v4u d = *reinterpret_cast<const avg_v4u*>(x + off);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const unsigned u = d[t];
                    ev[t] += __builtin_bit_cast(avg_s2, u << 8) >> 8;
                    od[t] += __builtin_bit_cast(avg_s2, u) >> 8;
                }
            }
        }
        const float div = (float)avg_divisor(g, w);
        avg_v4u o;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned b = avg_requant(ev[t].x, div, p.scale, p.lo) | (avg_requant(od[t].x, div, p.scale, p.lo) << 8) |
                               (avg_requant(ev[t].y, div, p.scale, p.lo) << 16) | (avg_requant(od[t].y, div, p.scale, p.lo) << 24);
            o[t] = b & avg_dword_mask(g, c.k, t);
        }
        *reinterpret_cast<avg_v4u*>(y + (size_t)i * 16) = o;
    }
}

static bool avg_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0) return false;
    if (2L * ph > kh || 2L * pw > kw) return false;
    return (long)kh * kw <= kAvgMaxTaps && shift >= -kAvgMaxShift && shift <= kAvgMaxShift;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_avgpool_i8_nhwc_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    return avg_supported(kh, kw, sh, sw, ph, pw, shift) ? 1 : 0;
}

extern "C" int fq_avgpool_i8_nhwc(const int8_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw,
                                  int ph, int pw, int count_include_pad, int shift, int relu, fq_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || Cpad <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return FQ_ERR_INVALID_ARG;
    if (C > Cpad || (Cpad & 15)) return FQ_ERR_INVALID_ARG;
    if (2L * ph > kh || 2L * pw > kw) return FQ_ERR_INVALID_ARG;         // torch's own constraint: no empty windows
    if ((long)H + 2L * ph < kh || (long)W + 2L * pw < kw) return FQ_ERR_INVALID_ARG;      // P < 1 or Q < 1
    const int P = avg_out_size(H, kh, sh, ph), Q = avg_out_size(W, kw, sw, pw);
    if (!avg_supported(kh, kw, sh, sw, ph, pw, shift)) return FQ_ERR_UNSUPPORTED;
    // 32-bit byte offsets in the kernel
    if ((long)N * H * W * Cpad >= 0x7fffffffL || (long)N * P * Q * Cpad >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (!x || !y || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u)) return FQ_ERR_INVALID_ARG;
    AvgParams p;
    AvgGeom& g = p.g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.Cpad = Cpad; g.CH = Cpad / 16; g.P = P; g.Q = Q;
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
    g.cip = count_include_pad ? 1 : 0;
    g.nchunks = (unsigned)((long)N * P * Q * g.CH);
    p.scale = ldexpf(1.0f, shift);
    p.lo = relu ? 0.0f : -128.0f;
    avgpool_i8_nhwc_kernel<<<(unsigned)avg_blocks(g), kAvgBlock, 0, as_stream(stream)>>>(x, y, p);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
