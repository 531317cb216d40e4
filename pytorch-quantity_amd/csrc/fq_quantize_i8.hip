// fq_quantize_i8.hip -- fp32 NCHW -> int8 NHWC with Quantity fused: the input of the integer convolutions (fq_conv_i8.hip).
//
//   quantize_i8_nhwc_kernel   x fp32 NCHW -> int8 NHWC (clamp(rint(x * 2^ib))), channels zero-padded
//                             to a multiple of 16.  HBM bound: 4 B read + 1 B written per element.
//   quantize_i8_unfold_w*     stem layers outside fq_conv2d_i8_stem's limits (fq_stem.hip): kernel width folded
//                             into the channel axis.
#include "fq_common.h"
#include "fq_int_tail.h"

namespace fq {

// ---- fp32 NCHW -> int8 NHWC with Quantity fused (new_quantity_op.py:52-58) -----------------------
// q8 (one element): fq_int_tail.h

// block = (64 hw) x (64 c) tile of one image.  Each thread loads a 4(c) x 4(hw) patch with four
// 16-byte loads along hw, quantises, and writes the patch transposed (4 dwords of 4 channels) into an
// LDS tile [hw][c]; the tile is then read back 16 channels at a time and stored with 16-byte stores.
// kVec = false: scalar loads for planes whose rows are not 16-byte aligned (HW % 4 != 0).
template <bool kVec>
__global__ __launch_bounds__(256) void quantize_i8_nhwc_kernel(const float* __restrict__ x, int8_t* __restrict__ y, int C, int HW,
                                                               int Cpad, float scale) {
    constexpr int RS = 17;                                // LDS row stride in dwords (64 c bytes + 4 pad)
    __shared__ unsigned tile[64 * RS];                    // [hw][c / 4]
    const int n = blockIdx.z, hw0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tid = threadIdx.x;
    const float* __restrict__ src = x + (long)n * C * HW;
    const int hwg = tid & 15, cg = tid >> 4;              // 16 hw groups of 4, 16 channel groups of 4
    const int hw = hw0 + 4 * hwg;
    float v[4][4];                                        // [channel i][hw e]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + 4 * cg + i;
        const bool c_ok = c < C;
        if (kVec) {
            const bool ok = c_ok && hw < HW;              // HW % 4 == 0: a group is all in or all out
            const float4 f = *reinterpret_cast<const float4*>(ok ? src + (long)c * HW + hw : src);
            v[i][0] = ok ? f.x : 0.0f; v[i][1] = ok ? f.y : 0.0f; v[i][2] = ok ? f.z : 0.0f; v[i][3] = ok ? f.w : 0.0f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = (c_ok && hw + e < HW) ? src[(long)c * HW + hw + e] : 0.0f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned packed = q8(v[0][e], scale) | (q8(v[1][e], scale) << 8) | (q8(v[2][e], scale) << 16) |
                                (q8(v[3][e], scale) << 24);
        tile[(4 * hwg + e) * RS + cg] = packed;
    }
    __syncthreads();
    // store: thread -> (hw = tid >> 2, 16 channels = tid & 3)
    const int shw = tid >> 2, cq = tid & 3;
    const int ohw = hw0 + shw, oc = c0 + 16 * cq;
    if (ohw < HW && oc < Cpad) {
        const unsigned* row = &tile[shw * RS + 4 * cq];
        int8_t* dst = y + ((long)n * HW + ohw) * Cpad + oc;
        if (oc + 16 <= Cpad && (Cpad & 15) == 0) {
            uint4 o; o.x = row[0]; o.y = row[1]; o.z = row[2]; o.w = row[3];
            *reinterpret_cast<uint4*>(dst) = o;
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (oc + 4 * d < Cpad) *reinterpret_cast<unsigned*>(dst + 4 * d) = row[d];
        }
    }
}

// C <= 4 (the image going into the stem convolution), Cpad == 16: one pixel per thread -- C coalesced
// plane reads, one 16-byte store of [c0 c1 c2 c3 0 ... 0].
__global__ __launch_bounds__(256) void quantize_i8_nhwc_smallc_kernel(const float* __restrict__ x, int8_t* __restrict__ y, int C,
                                                                      int HW, long total_pixels, float scale) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    for (; i < total_pixels; i += stride) {
        const long n = i / HW;
        const int hw = (int)(i - n * HW);
        const float* __restrict__ src = x + n * C * HW + hw;
        unsigned packed = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) packed |= q8(src[(long)c * HW], scale) << (8 * c);
        uint4 o; o.x = packed; o.y = 0; o.z = 0; o.w = 0;
        *reinterpret_cast<uint4*>(y + i * 16) = o;
    }
}

// Stem layers (C <= 4, e.g. 7x7 stride-2 on RGB): channel padding to 16 would waste 13/16 of every
// MFMA.  Instead the kernel width is folded into the channel axis: y[n][ih][q][s*C + c] =
// Quantity(x[n][c][ih][q*stride_w - pad_w + s*dil_w]) (zero outside the image / beyond S*C), Cpad2 bytes
// per output column q.  The convolution then runs with S = 1, stride_w = 1, pad_w = 0 over width Q and
// "channels" Cpad2: an R x 1 kernel with R * Cpad2 reduction bytes instead of R * S * 16.
__global__ __launch_bounds__(256) void quantize_i8_unfold_w_kernel(const float* __restrict__ x, int8_t* __restrict__ y, int C, int H,
                                                                   int W, int S, int stride_w, int pad_w, int dil_w, int Q,
                                                                   int Cpad2, long total, float scale) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    for (; i < total; i += stride) {                      // i = (n*H + ih)*Q + q
        const int q = (int)(i % Q);
        const long nih = i / Q;
        const int ih = (int)(nih % H);
        const long n = nih / H;
        const float* __restrict__ src = x + (n * C * H + ih) * (long)W;     // + c*H*W + iw
        int8_t* dst = y + i * Cpad2;
        const int iw0 = q * stride_w - pad_w;
        for (int b0 = 0; b0 < Cpad2; b0 += 4) {           // one dword (4 folded channels) at a time
            unsigned packed = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = b0 + e;                      // folded channel = s*C + c
                const int s_ = f / C, c = f - s_ * C;
                const int iw = iw0 + s_ * dil_w;
                if (s_ < S && (unsigned)iw < (unsigned)W) packed |= q8(src[(long)c * H * W + iw], scale) << (8 * e);
            }
            *reinterpret_cast<unsigned*>(dst + b0) = packed;
        }
    }
}

// The common stem (C <= 4 channels, S <= 8 taps, S*C <= 32 folded channels): C is a template parameter and
// the tap loop is fully unrolled, so every folded-channel index is a compile-time constant -- no division per
// element, the 32 output bytes are assembled in registers and leave as two 16-byte stores.  Neighbouring
// threads (q, q+1) read overlapping input columns, which the L1 absorbs.
template <int C>
__global__ __launch_bounds__(256) void quantize_i8_unfold_w_small_kernel(const float* __restrict__ x, int8_t* __restrict__ y, int H, int W,
                                                                         int S, int stride_w, int pad_w, int dil_w, int Q, int Cpad2,
                                                                         long total, float scale) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    const long plane = (long)H * W;
    for (; i < total; i += stride) {                      // i = (n*H + ih)*Q + q
        const int q = (int)(i % Q);
        const long nih = i / Q;
        const int ih = (int)(nih % H);
        const long n = nih / H;
        const float* __restrict__ src = x + (n * C * H + ih) * (long)W;     // + c*H*W + iw
        const int iw0 = q * stride_w - pad_w;
        unsigned out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s_ = 0; s_ < 8; ++s_) {
            const int iw = iw0 + s_ * dil_w;
            const bool ok = s_ < S && (unsigned)iw < (unsigned)W;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int f = s_ * C + c;                  // compile-time after unrolling
                const float v = ok ? src[c * plane + iw] : 0.0f;
                out[f >> 2] |= q8(v, scale) << (8 * (f & 3));
            }
        }
        int8_t* dst = y + i * Cpad2;
        uint4 o0; o0.x = out[0]; o0.y = out[1]; o0.z = out[2]; o0.w = out[3];
        *reinterpret_cast<uint4*>(dst) = o0;
        if (Cpad2 > 16) {
            uint4 o1; o1.x = out[4]; o1.y = out[5]; o1.z = out[6]; o1.w = out[7];
            *reinterpret_cast<uint4*>(dst + 16) = o1;
        }
    }
}

// HW == 1 (Linear input [N][F]): layouts coincide, plain element-wise with channel padding
__global__ __launch_bounds__(256) void quantize_i8_rows_kernel(const float* __restrict__ x, int8_t* __restrict__ y, int C, int Cpad,
                                                               long rows, float scale) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = rows * Cpad, stride = (long)gridDim.x * 256;
    for (; i < total; i += stride) {
        const long rrow = i / Cpad;
        const int c = (int)(i - rrow * Cpad);
        float v = c < C ? x[rrow * C + c] : 0.0f;
        float q = rintf(v * scale);
        q = q < -128.0f ? -128.0f : (q > 127.0f ? 127.0f : q);
        y[i] = (int8_t)(int)q;
    }
}

}  // namespace fq

using namespace fq;

extern "C" int fq_quantize_i8_nhwc(const float* x_nchw, int8_t* y_nhwc, int N, int C, int HW, int Cpad, int ib,
                                   fq_stream_t stream) {
    if (N < 0 || C <= 0 || HW < 0 || Cpad < C || (Cpad & 3) || ib < -120 || ib > 120) return FQ_ERR_INVALID_ARG;
    if (N == 0 || HW == 0) return FQ_OK;
    if (!x_nchw || !y_nhwc) return FQ_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(y_nhwc) & 3u) return FQ_ERR_INVALID_ARG;
    hipStream_t st = as_stream(stream);
    const float scale = ldexpf(1.0f, ib);
    if (HW == 1) {
        const long total = (long)N * Cpad;
        long g = (total + 255) / 256;
        if (g > kCUs * 16) g = kCUs * 16;
        hipLaunchKernelGGL(quantize_i8_rows_kernel, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y_nhwc, C, Cpad, (long)N, scale);
    } else if (C <= 4 && Cpad == 16 && (reinterpret_cast<uintptr_t>(y_nhwc) & 15u) == 0) {
        const long total = (long)N * HW;
        long g = (total + 255) / 256;
        if (g > kCUs * 32) g = kCUs * 32;
        hipLaunchKernelGGL(quantize_i8_nhwc_smallc_kernel, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y_nhwc, C, HW, total, scale);
    } else {
        if (N > 65535) return FQ_ERR_UNSUPPORTED;
        dim3 grid((HW + 63) / 64, (Cpad + 63) / 64, N);
        const bool vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(x_nchw) & 15u) == 0);
        if (vec)
            hipLaunchKernelGGL(quantize_i8_nhwc_kernel<true>, grid, dim3(256), 0, st, x_nchw, y_nhwc, C, HW, Cpad, scale);
        else
            hipLaunchKernelGGL(quantize_i8_nhwc_kernel<false>, grid, dim3(256), 0, st, x_nchw, y_nhwc, C, HW, Cpad, scale);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

extern "C" int fq_quantize_i8_unfold_w(const float* x_nchw, int8_t* y, int N, int C, int H, int W, int S, int stride_w,
                                       int pad_w, int dil_w, int Cpad2, int ib, fq_stream_t stream) {
    if (N < 0 || C <= 0 || H <= 0 || W <= 0 || S <= 0 || stride_w <= 0 || pad_w < 0 || dil_w <= 0 || ib < -120 || ib > 120)
        return FQ_ERR_INVALID_ARG;
    if (Cpad2 < S * C || (Cpad2 & 15)) return FQ_ERR_INVALID_ARG;
    const int Q = (W + 2 * pad_w - dil_w * (S - 1) - 1) / stride_w + 1;
    if (Q <= 0) return FQ_ERR_INVALID_ARG;
    if (N == 0) return FQ_OK;
    if (!x_nchw || !y || (reinterpret_cast<uintptr_t>(y) & 15u)) return FQ_ERR_INVALID_ARG;
    const long total = (long)N * H * Q;
    long g = (total + 255) / 256;
    if (g > kCUs * 32) g = kCUs * 32;
    const float scale = ldexpf(1.0f, ib);
    hipStream_t st = as_stream(stream);
    if (C <= 4 && S <= 8 && S * C <= 32 && Cpad2 <= 32) {
        switch (C) {
            case 1: hipLaunchKernelGGL(quantize_i8_unfold_w_small_kernel<1>, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y, H, W, S,
                                       stride_w, pad_w, dil_w, Q, Cpad2, total, scale); break;
            case 2: hipLaunchKernelGGL(quantize_i8_unfold_w_small_kernel<2>, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y, H, W, S,
                                       stride_w, pad_w, dil_w, Q, Cpad2, total, scale); break;
            case 3: hipLaunchKernelGGL(quantize_i8_unfold_w_small_kernel<3>, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y, H, W, S,
                                       stride_w, pad_w, dil_w, Q, Cpad2, total, scale); break;
            default: hipLaunchKernelGGL(quantize_i8_unfold_w_small_kernel<4>, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y, H, W, S,
                                        stride_w, pad_w, dil_w, Q, Cpad2, total, scale); break;
        }
    } else {
        hipLaunchKernelGGL(quantize_i8_unfold_w_kernel, dim3((unsigned)g), dim3(256), 0, st, x_nchw, y, C, H, W, S, stride_w, pad_w,
                           dil_w, Q, Cpad2, total, scale);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
