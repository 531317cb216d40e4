// fq_avgpool_i16.hip -- windowed nn.AvgPool2d on the exact int16 NHWC sum of a resident NewAdd, re-quantised for the convolution
// behind it (include/fq.h: fq_avgpool_i16_nhwc).  The ResNet-D shortcut: AvgPool2d(2, 2) -> 1x1 convolution reading ReLU(sum).
//
// The rule is fq_avgpool_i8_nhwc's, word for word (fq_avgpool_i8.hip): per output element and channel
//   S = sum of x over window ∩ image (int32), D = kh kw (count_include_pad) or the number of taps inside the image,
//   f = (float)S / (float)D           ONE correctly rounded fp32 division
//   t = f * 2^(b - g)                 exact
//   y = clamp(relu ? max(rint(t), 0) : rint(t), -128, 127)          rint: half to even
// It stays the reference's chain DeQuantity(g) -> nn.AvgPool2d -> nn.ReLU -> Quantity(b) for ANY int16 source:
// |S| <= 64 * 32768 = 2^21 < 2^24, so every partial sum of torch's fp32 accumulation and the conversion (float)S are exact.
// A bandwidth kernel without LDS, shaped like avgpool_i8_nhwc_kernel:
//   * one lane owns 8 consecutive channels of one output pixel (fq_avgpool_i16_geom.h): ONE dwordx4 load per tap, contiguous
//     across the wave (1 KiB), and one dwordx2 store (512 contiguous bytes per wave).  Chosen over 16 channels per lane (two
//     loads per tap, one dwordx4 store): half the int32 accumulators and half the correctly rounded divisions per lane -- a
//     division is some twenty VALU instructions, sixteen of them per item were the int8 kernel's longest stretch --, twice the
//     work items where the plane is small (the last stage of a ResNet-D: 7 x 7 outputs), and both widths sit in the 8 to 16
//     bytes per lane at which loads and stores coalesce fully;
//   * at most 2048 workgroups of 256 lanes, every lane steps through the items by the grid size;
//   * the window is cut to the image once per output pixel, so a tap outside it is skipped, never clamped;
//   * the two int16 of a dword are sign-extended with one shift pair each and accumulated in int32 (packed int16 no longer
//     holds S);
//   * eight plain `/` divisions per item (the build has -fhip-fp32-correctly-rounded-divide-sqrt and no fast-math), the exact
//     power of two, rintf, ReLU and clamp folded into one fmaxf / fminf pair; channels at and above C are masked to zero whatever
//     the source's padding channels hold.
// Every load is 16-byte aligned and lies inside [x, x + 2 N H W Cpad); scripts/avgpool_i16_geom_check.cpp walks the same
// functions on the host over the tests' shapes.
#include "fq_common.h"
#include "fq_avgpool_i16_geom.h"

namespace fq {

struct Avg16Params {
    AvgGeom g;
    float scale;                       // 2^shift
    float lo;                          // 0 with the fused ReLU, else -128
};

typedef unsigned avg16_v4u __attribute__((ext_vector_type(4)));
typedef unsigned avg16_v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned avg16_requant(int s, float d, float scale, float lo) {
    const float r = rintf(((float)s / d) * scale);
    return (unsigned)(int)fminf(fmaxf(r, lo), 127.0f) & 0xffu;
}

__global__ __launch_bounds__(kAvgBlock) void avgpool_i16_nhwc_kernel(const int16_t* __restrict__ x, int8_t* __restrict__ y,
                                                                      const Avg16Params p) {
    const AvgGeom& g = p.g;
    const unsigned stride = gridDim.x * kAvgBlock;
    const unsigned step = avg16_tap_step(g);
    const char* xb = reinterpret_cast<const char*>(x);
    for (unsigned i = blockIdx.x * kAvgBlock + threadIdx.x; i < g.nchunks; i += stride) {
        const AvgChunk c = avg_chunk(g, i);
        const AvgWindow w = avg_window(g, c.p, c.q);
        int s[kAvg16Lane];
#pragma unroll
        for (int t = 0; t < kAvg16Lane; ++t) s[t] = 0;
        for (int ih = w.h0; ih < w.h1; ++ih) {
            unsigned off = avg16_tap_offset(g, c.n, ih, w.w0, c.k);
            for (int iw = w.w0; iw < w.w1; ++iw, off += step) {
                const avg16_v4u d = *reinterpret_cast<const avg16_v4u*>(xb + off);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s[2 * t] += (int)(d[t] << 16) >> 16;
                    s[2 * t + 1] += (int)d[t] >> 16;
                }
            }
        }
        const float div = (float)avg_divisor(g, w);
        avg16_v2u o;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned b = avg16_requant(s[4 * t], div, p.scale, p.lo) | (avg16_requant(s[4 * t + 1], div, p.scale, p.lo) << 8) |
                               (avg16_requant(s[4 * t + 2], div, p.scale, p.lo) << 16) |
                               (avg16_requant(s[4 * t + 3], div, p.scale, p.lo) << 24);
            o[t] = b & avg16_dword_mask(g, c.k, t);
        }
        *reinterpret_cast<avg16_v2u*>(y + avg16_store_offset(i)) = o;
    }
}

static bool avg16_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0) return false;
    if (2L * ph > kh || 2L * pw > kw) return false;
    return (long)kh * kw <= kAvgMaxTaps && shift >= -kAvgMaxShift && shift <= kAvgMaxShift;
}

// true when the product a b c d e of non-negative ints is at or above `limit`; compared factor by factor, so nothing overflows
static bool avg16_bytes_reach(long limit, int a, int b, int c, int d, int e) {
    const int f[5] = {a, b, c, d, e};
    long v = 1;
    for (int i = 0; i < 5; ++i) {
        if (f[i] == 0) return false;
        if (v >= (limit + f[i] - 1) / f[i]) return true;
        v *= f[i];
    }
    return v >= limit;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_avgpool_i16_nhwc_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    return avg16_supported(kh, kw, sh, sw, ph, pw, shift) ? 1 : 0;
}

extern "C" int fq_avgpool_i16_nhwc(const int16_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw,
                                   int ph, int pw, int count_include_pad, int shift, int relu, fq_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || Cpad <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return FQ_ERR_INVALID_ARG;
    if (C > Cpad || (Cpad & 15)) return FQ_ERR_INVALID_ARG;
    if (2L * ph > kh || 2L * pw > kw) return FQ_ERR_INVALID_ARG;         // torch's own constraint: no empty windows
    if ((long)H + 2L * ph < kh || (long)W + 2L * pw < kw) return FQ_ERR_INVALID_ARG;      // P < 1 or Q < 1
    const int P = avg_out_size(H, kh, sh, ph), Q = avg_out_size(W, kw, sw, pw);
    if (!avg16_supported(kh, kw, sh, sw, ph, pw, shift)) return FQ_ERR_UNSUPPORTED;
    // 32-bit byte offsets in the kernel: the source has 2 N H W Cpad bytes, the output N P Q Cpad
    if (avg16_bytes_reach(0x7fffffffL, 2, N, H, W, Cpad) || avg16_bytes_reach(0x7fffffffL, 1, N, P, Q, Cpad)) return FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (!x || !y || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u)) return FQ_ERR_INVALID_ARG;
    Avg16Params p;
    p.g = avg16_geom(N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, count_include_pad);
    p.scale = ldexpf(1.0f, shift);
    p.lo = relu ? 0.0f : -128.0f;
    avgpool_i16_nhwc_kernel<<<(unsigned)avg_blocks(p.g), kAvgBlock, 0, as_stream(stream)>>>(x, y, p);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
