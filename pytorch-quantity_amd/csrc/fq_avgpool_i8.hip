// fq_avgpool_i8.hip -- windowed nn.AvgPool2d on a resident NHWC activation, re-quantised for the convolution behind it, for two
// sources on one skeleton (include/fq.h): fq_avgpool_i8_nhwc reads an int8 activation, fq_avgpool_i16_nhwc the exact int16 sum of
// a resident NewAdd (the ResNet-D shortcut: AvgPool2d(2, 2) -> 1x1 convolution reading ReLU(sum)).
//
// The reference's chain is DeQuantity(g) -> nn.AvgPool2d -> optional nn.ReLU -> Quantity(b) of the consumer.  The source holds
// integers on the grid g, so every partial sum of torch's fp32 accumulation is exact and the chain is, per output element and
// channel,
//   S = sum of x over window ∩ image (int), D = kh kw (count_include_pad) or the number of taps inside the image,
//   f = (float)S / (float)D           ONE correctly rounded fp32 division
//   t = f * 2^(b - g)                 exact
//   y = clamp(relu ? max(rint(t), 0) : rint(t), -128, 127)          rint: half to even
// -- two roundings on purpose (f to fp32, then t to an integer): rounding the rational S 2^shift / D once is another function.
// At most 64 taps (kAvgMaxTaps): |S| <= 64 * 128 = 8192 for int8, which a packed int16 lane holds, and <= 64 * 32768 = 2^21 < 2^24
// for ANY int16 source, so the int32 sum, torch's partial sums and the conversion (float)S are exact there too.
// A bandwidth kernel without LDS:
//   * one lane owns one item of the output (fq_avgpool_i8_geom.h), channel fastest, so a wave loads and stores whole contiguous
//     pixels; at most 2048 workgroups of 256 lanes, every lane steps through the items by the grid size;
//   * ONE dwordx4 load per tap for either source: 16 int8 channels, stored with one dwordx4, or 8 int16 channels, stored with one
//     dwordx2.  The int16 lane is 8 channels wide and not 16 (two loads per tap, one dwordx4 store): half the int32 accumulators
//     and half the correctly rounded divisions per lane -- a division is some twenty VALU instructions, sixteen of them per item
//     are the int8 kernel's longest stretch --, twice the work items where the plane is small (the last stage of a ResNet-D:
//     7 x 7 outputs), and both widths sit in the 8 to 16 bytes per lane at which loads and stores coalesce fully;
//   * the window is cut to the image once per output pixel, so a tap outside it is skipped, never clamped;
//   * int8: bytes are sign-extended two at a time into packed int16 lanes (even bytes: shift up by 8, then a packed arithmetic
//     shift down; odd bytes: the packed shift alone) and accumulated with packed adds.  int16: the two halves of a dword are
//     sign-extended with one shift pair each and accumulated in int32 (packed int16 no longer holds S);
//   * one plain `/` division per channel (the build has -fhip-fp32-correctly-rounded-divide-sqrt and no fast-math), the exact
//     power of two, rintf, ReLU and clamp folded into one fmaxf / fminf pair; channels at and above C are masked to zero whatever
//     the source's padding channels hold.
// Every load is 16-byte aligned and lies inside the source's Src::kBytes N H W Cpad bytes; scripts/avgpool_geom_check.cpp walks
// the same functions on the host over the tests' shapes, for both sources.
#include "fq_common.h"
#include "fq_avgpool_i8_geom.h"

namespace fq {

struct AvgParams {
    AvgGeom g;
    float scale;                       // 2^shift
    float lo;                          // 0 with the fused ReLU, else -128
};

typedef unsigned avg_v4u __attribute__((ext_vector_type(4)));
typedef unsigned avg_v2u __attribute__((ext_vector_type(2)));
typedef short avg_s2 __attribute__((ext_vector_type(2)));

// What the skeleton asks of a source beyond the geometry's constants: the running sums of a lane's channels, how the 16 bytes of
// a tap are added to them, sum j of the lane (j = 0 ... kLane - 1, channel order), and the store of the item's dwords.
struct AvgI8 : AvgSrcI8 {
    typedef int8_t elem;
    typedef avg_s2 Acc[8];                                // [t]: bytes 0, 2 of dword t; [4 + t]: bytes 1, 3
    static __device__ __forceinline__ void add(Acc& a, const avg_v4u d) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned u = d[t];
            a[t] += __builtin_bit_cast(avg_s2, u << 8) >> 8;
            a[4 + t] += __builtin_bit_cast(avg_s2, u) >> 8;
        }
    }
    static __device__ __forceinline__ int sum(const Acc& a, int j) {
        const avg_s2 v = a[4 * (j & 1) + (j >> 2)];
        return (j & 2) ? v.y : v.x;
    }
    typedef avg_v4u Out;                                  // the item's 16 output bytes: one dwordx4 store
};

struct AvgI16 : AvgSrcI16 {
    typedef int16_t elem;
    typedef int Acc[8];
    static __device__ __forceinline__ void add(Acc& s, const avg_v4u d) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[2 * t] += (int)(d[t] << 16) >> 16;
            s[2 * t + 1] += (int)d[t] >> 16;
        }
    }
    static __device__ __forceinline__ int sum(const Acc& s, int j) { return s[j]; }
    typedef avg_v2u Out;                                  // 8 output bytes: one dwordx2 store
};

__device__ __forceinline__ unsigned avg_requant(int s, float d, float scale, float lo) {
    const float r = rintf(((float)s / d) * scale);
    return (unsigned)(int)fminf(fmaxf(r, lo), 127.0f) & 0xffu;
}

template <class Src>
__global__ __launch_bounds__(kAvgBlock) void avgpool_nhwc_kernel(const typename Src::elem* __restrict__ x, int8_t* __restrict__ y,
                                                                  const AvgParams p) {
    const AvgGeom& g = p.g;
    const unsigned stride = gridDim.x * kAvgBlock;
    const unsigned step = avg_tap_step<Src>(g);
    const char* xb = reinterpret_cast<const char*>(x);
    for (unsigned i = blockIdx.x * kAvgBlock + threadIdx.x; i < g.nchunks; i += stride) {
        const AvgChunk c = avg_chunk(g, i);
        const AvgWindow w = avg_window(g, c.p, c.q);
        typename Src::Acc a;
#pragma unroll
        for (unsigned t = 0; t < sizeof(a) / sizeof(a[0]); ++t) a[t] = {};
        for (int ih = w.h0; ih < w.h1; ++ih) {
            unsigned off = avg_tap_offset<Src>(g, c.n, ih, w.w0, c.k);
            for (int iw = w.w0; iw < w.w1; ++iw, off += step) Src::add(a, *reinterpret_cast<const avg_v4u*>(xb + off));
        }
        const float div = (float)avg_divisor(g, w);
        typename Src::Out o;
#pragma unroll
        for (int t = 0; t < Src::kOutBytes / 4; ++t) {
            const unsigned b = avg_requant(Src::sum(a, 4 * t), div, p.scale, p.lo) | (avg_requant(Src::sum(a, 4 * t + 1), div, p.scale, p.lo) << 8) |
                               (avg_requant(Src::sum(a, 4 * t + 2), div, p.scale, p.lo) << 16) |
                               (avg_requant(Src::sum(a, 4 * t + 3), div, p.scale, p.lo) << 24);
            o[t] = b & avg_dword_mask<Src>(g, c.k, t);
        }
        *reinterpret_cast<typename Src::Out*>(y + avg_store_offset<Src>(i)) = o;
    }
}

static bool avg_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0) return false;
    if (2L * ph > kh || 2L * pw > kw) return false;
    return (long)kh * kw <= kAvgMaxTaps && shift >= -kAvgMaxShift && shift <= kAvgMaxShift;
}

// true when the product a b c d e of non-negative ints is at or above `limit`; compared factor by factor, so nothing overflows
static bool avg_bytes_reach(long limit, int a, int b, int c, int d, int e) {
    const int f[5] = {a, b, c, d, e};
    long v = 1;
    for (int i = 0; i < 5; ++i) {
        if (f[i] == 0) return false;
        if (v >= (limit + f[i] - 1) / f[i]) return true;
        v *= f[i];
    }
    return v >= limit;
}

template <class Src>
static int avg_run(const typename Src::elem* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw, int ph,
                   int pw, int count_include_pad, int shift, int relu, fq_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || Cpad <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return FQ_ERR_INVALID_ARG;
    if (C > Cpad || (Cpad & 15)) return FQ_ERR_INVALID_ARG;
    if (2L * ph > kh || 2L * pw > kw) return FQ_ERR_INVALID_ARG;         // torch's own constraint: no empty windows
    if ((long)H + 2L * ph < kh || (long)W + 2L * pw < kw) return FQ_ERR_INVALID_ARG;      // P < 1 or Q < 1
    const int P = avg_out_size(H, kh, sh, ph), Q = avg_out_size(W, kw, sw, pw);
    if (!avg_supported(kh, kw, sh, sw, ph, pw, shift)) return FQ_ERR_UNSUPPORTED;
    // 32-bit byte offsets in the kernel: the source has kBytes N H W Cpad bytes, the output N P Q Cpad
    if (avg_bytes_reach(0x7fffffffL, Src::kBytes, N, H, W, Cpad) || avg_bytes_reach(0x7fffffffL, 1, N, P, Q, Cpad)) return FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (!x || !y || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u)) return FQ_ERR_INVALID_ARG;
    AvgParams p;
    p.g = avg_geom<Src>(N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, count_include_pad);
    p.scale = ldexpf(1.0f, shift);
    p.lo = relu ? 0.0f : -128.0f;
    avgpool_nhwc_kernel<Src><<<(unsigned)avg_blocks(p.g), kAvgBlock, 0, as_stream(stream)>>>(x, y, p);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_avgpool_i8_nhwc_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    return avg_supported(kh, kw, sh, sw, ph, pw, shift) ? 1 : 0;
}

extern "C" int fq_avgpool_i16_nhwc_supported(int kh, int kw, int sh, int sw, int ph, int pw, int shift) {
    return avg_supported(kh, kw, sh, sw, ph, pw, shift) ? 1 : 0;
}

extern "C" int fq_avgpool_i8_nhwc(const int8_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw,
                                  int ph, int pw, int count_include_pad, int shift, int relu, fq_stream_t stream) {
    return avg_run<AvgI8>(x, y, N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, count_include_pad, shift, relu, stream);
}

extern "C" int fq_avgpool_i16_nhwc(const int16_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw,
                                   int ph, int pw, int count_include_pad, int shift, int relu, fq_stream_t stream) {
    return avg_run<AvgI16>(x, y, N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, count_include_pad, shift, relu, stream);
}
