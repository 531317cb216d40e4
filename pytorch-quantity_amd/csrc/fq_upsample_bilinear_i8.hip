// fq_upsample_bilinear_i8.hip -- nn.Upsample(scale_factor=2 or 4, mode="bilinear", align_corners=False) on a resident int8 NHWC
// activation, re-quantised for the convolutions behind it (include/fq.h: fq_upsample_bilinear_i8_nhwc).
//
// The reference's chain is DeQuantity(g) -> bilinear interpolation -> optional nn.ReLU -> Quantity(b) of the consumers.  The
// interpolation weights are odd multiples of 1 / D, D = 2 up, and the source is int8 on the grid g, so every product and partial
// sum of torch's fp32 kernel is a dyadic number of at most 14 significant bits: exact in any order.  Per output element
//   S = sum over the 2 x 2 taps of ly lx q        (|S| <= 128 D^2)
//   r = S * 2^(b - g - 2 log2 D)                   rounded half to even, ONE rounding, in integers
//   y = clamp(relu ? max(r, 0) : r, -128, 127)
// -- no fp32 step at all (the average pool has one: its divisor is no power of two).
// The kernel is store-bound (1 byte read, up^2 written) and has no LDS:
//   * one lane owns 16 channels of one SOURCE pixel (fq_upsample_bilinear_i8_geom.h) and writes its up x up output pixels; the taps
//     of all of them lie in the pixel's 3 x 3 neighbourhood with indices clamped to the plane: nine dwordx4 loads, eight of which
//     the neighbouring lanes and rows load too (L1 / L2 hits), for 4 or 16 dwordx4 stores;
//   * consecutive lanes walk the channels of a pixel, then the pixels of a row: the `up` stores of one output row together cover
//     contiguous bytes;
//   * bytes are sign-extended two at a time into packed int16 (as fq_avgpool_i8.hip does); the interpolation is separable: the
//     row pass (|.| <= 128 D) once per dy for the three columns, the column pass (|S| <= 8192) per output, weights compile-time
//     constants; the rounding adds 2^(k-1) - 1 and the bit that becomes the lowest, then shifts, all in packed int16 (the largest
//     intermediate is 16384); for b - g >= 2 log2 D the sum is clamped to int8 first and shifted left; for b - g <= 0 the result
//     cannot leave int8 and the clamp is left out (upb_requant_pk's MODE), the ReLU a compile-time flag: twelve instantiations;
//   * channels at and above C are masked to zero whatever the source's padding channels hold;
//   * at most 4096 workgroups of 256 lanes; a lane's first item is split by division, every further one digit by digit.
// Every load is 16-byte aligned and lies inside [x, x + N H W Cpad); scripts/upsample_bilinear_geom_check.cpp walks the same
// functions on the host.
#include "fq_common.h"
#include "fq_upsample_bilinear_i8_geom.h"

namespace fq {

typedef unsigned upb_v4u __attribute__((ext_vector_type(4)));
typedef short upb_s2 __attribute__((ext_vector_type(2)));

// MODE 0: a rounding right shift with shift = b - g <= 0 -- |r| <= 128 * 2^shift and r = 128 cannot occur (S <= 127 D^2), so no clamp
// is needed, only the ReLU's max; MODE 1: a rounding right shift that can leave int8 (0 < shift < 2 log2 D); MODE 2: e >= 0, a
// clamp to int8 first and an exact left shift.
template <int MODE, bool RELU>
__device__ __forceinline__ upb_s2 upb_requant_pk(upb_s2 s, const upb_s2 sh, const upb_s2 bias) {
    const upb_s2 one = {1, 1}, hi = {127, 127}, m128 = {-128, -128}, zero = {0, 0};
    upb_s2 v;
    if constexpr (MODE == 2) {
        v = __builtin_elementwise_min(__builtin_elementwise_max(s, m128), hi) << sh;
    } else {
        v = (s + bias + ((s >> sh) & one)) >> sh;
    }
    if constexpr (MODE == 0) return RELU ? __builtin_elementwise_max(v, zero) : v;
    return __builtin_elementwise_min(__builtin_elementwise_max(v, RELU ? zero : m128), hi);
}

template <int UP, int MODE, bool RELU>
__global__ __launch_bounds__(kUpbBlock) void upsample_bilinear_i8_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                        const UpbGeom g, const UpbRound r) {
    unsigned i = blockIdx.x * kUpbBlock + threadIdx.x;
    if (i >= g.items) return;
    const unsigned stride = gridDim.x * kUpbBlock;
    const short shv = (short)(MODE == 2 ? r.lsh : r.rsh);
    const upb_s2 sh = {shv, shv}, bias = {(short)r.bias, (short)r.bias};
    UpbItem c = upb_first(g, i);
    for (;;) {
        const UpbNbr nb = upb_nbr(g, c);
        upb_s2 src[3][3][8];                              // [row][col][2 t: bytes 0, 2 of dword t; 2 t + 1: bytes 1, 3]
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const upb_v4u d = *reinterpret_cast<const upb_v4u*>(x + upb_src_offset(g, c.n, nb.row[a], nb.col[b], c.k));
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const unsigned u = d[t];
                    src[a][b][2 * t] = __builtin_bit_cast(upb_s2, u << 8) >> 8;
                    src[a][b][2 * t + 1] = __builtin_bit_cast(upb_s2, u) >> 8;
                }
            }
        }
        unsigned mask[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) mask[t] = upb_dword_mask(g, c.k, t);
#pragma unroll
        for (int dy = 0; dy < UP; ++dy) {
            const UpbTap ty = upb_tap(UP, dy);
            upb_s2 v[3][8];                               // the row pass for the three columns
#pragma unroll
            for (int b = 0; b < 3; ++b) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[b][j] = src[ty.first][b][j] * (short)ty.l0 + src[ty.first + 1][b][j] * (short)ty.l1;
            }
#pragma unroll
            for (int dx = 0; dx < UP; ++dx) {
                const UpbTap tx = upb_tap(UP, dx);
                upb_v4u o;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const upb_s2 ev = upb_requant_pk<MODE, RELU>(v[tx.first][2 * t] * (short)tx.l0 + v[tx.first + 1][2 * t] * (short)tx.l1,
                                                                 sh, bias);
                    const upb_s2 od = upb_requant_pk<MODE, RELU>(v[tx.first][2 * t + 1] * (short)tx.l0 + v[tx.first + 1][2 * t + 1] * (short)tx.l1,
                                                                 sh, bias);
                    o[t] = ((__builtin_bit_cast(unsigned, ev) & 0x00ff00ffu) | ((__builtin_bit_cast(unsigned, od) & 0x00ff00ffu) << 8)) & mask[t];
                }
                *reinterpret_cast<upb_v4u*>(y + upb_dst_offset(g, c, dy, dx)) = o;
            }
        }
        i += stride;
        if (i >= g.items) break;
        c = upb_next(g, c);
    }
}

template <int UP, int MODE>
static void upb_launch_mode(hipStream_t st, const int8_t* x, int8_t* y, const UpbGeom& g, const UpbRound& r) {
    const unsigned blocks = upb_blocks(g.items);
    if (r.lo == 0) upsample_bilinear_i8_kernel<UP, MODE, true><<<blocks, kUpbBlock, 0, st>>>(x, y, g, r);
    else upsample_bilinear_i8_kernel<UP, MODE, false><<<blocks, kUpbBlock, 0, st>>>(x, y, g, r);
}

template <int UP>
static void upb_launch(hipStream_t st, const int8_t* x, int8_t* y, const UpbGeom& g, const UpbRound& r, int shift) {
    if (r.rsh == 0) upb_launch_mode<UP, 2>(st, x, y, g, r);
    else if (shift <= 0) upb_launch_mode<UP, 0>(st, x, y, g, r);
    else upb_launch_mode<UP, 1>(st, x, y, g, r);
}

}  // namespace fq

using namespace fq;

extern "C" int fq_upsample_bilinear_i8_nhwc_supported(int up, int shift) { return upb_supported(up, shift) ? 1 : 0; }

extern "C" int fq_upsample_bilinear_i8_nhwc(const int8_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int up, int shift,
                                            int relu, fq_stream_t stream) {
    const int rc = upb_args(N, H, W, C, Cpad, up, shift);
    if (rc) return rc == -1 ? FQ_ERR_INVALID_ARG : FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (!x || !y || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u)) return FQ_ERR_INVALID_ARG;
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), yb = reinterpret_cast<uintptr_t>(y);
    const uintptr_t xn = (uintptr_t)((long)N * H * W * Cpad), yn = xn * (uintptr_t)(up * up);
    if (xb < yb + yn && yb < xb + xn) return FQ_ERR_INVALID_ARG;          // y overlaps x
    const UpbGeom g = upb_geom(N, H, W, C, Cpad, up);
    const UpbRound r = upb_round(up, shift, relu);
    hipStream_t st = as_stream(stream);
    if (up == 2) upb_launch<2>(st, x, y, g, r, shift);
    else upb_launch<4>(st, x, y, g, r, shift);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
