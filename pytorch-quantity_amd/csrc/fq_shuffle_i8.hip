// fq_shuffle_i8.hip -- channel shuffle (nn.ChannelShuffle) and channel slice (the Slice marker) of resident int8 NHWC
// activations (include/fq.h: fq_shuffle_i8_nhwc).
//
//   y[n][h][w][j] = x[n][h][w][c_off + (j mod g) * (C / g) + floor(j / g)]     0 <= j < C
//                 = 0                                                           C <= j < Cpad_out
//
// A permutation of the integers is the same permutation of the values q * 2^-grid: no arithmetic at all, one read of the
// span of every source row and one write of every output row.
//   * a workgroup takes a TILE of pixels (fq_shuffle_i8_geom.h): it stages the 16-byte-aligned span [a0, a0 + S) of each of
//     the tile's source rows in LDS with dwordx4 loads -- stage item i goes to LDS byte 16 i, so both sides are linear in the
//     lane -- and after a barrier every lane assembles whole 16-byte units of the output rows from LDS bytes and stores them
//     with one dwordx4, unit index fastest, so a wave stores contiguous pixels;
//   * the bytes of a unit are walked with one division (shuf_walk_begin) and increments; bytes j >= C are zero without a read,
//     so neither the source's padding channels nor anything behind the span reaches the output;
//   * at most 2048 workgroups; a workgroup strides over the remaining tiles (two barriers per tile);
//   * a span above the LDS budget (C above about 32 K: no network has one) is not staged: the same walk reads the bytes of the
//     source row from global memory (LDS == false).  Byte loads are aligned loads.
// Every global load lies inside [x, x + N H W Cpad_in): a0 + S <= Cpad_in because Cpad_in % 16 == 0, and pixels past the last
// one are neither staged nor written.  scripts/shuffle_geom_check.cpp walks the same functions on the host over the tests' shapes.
#include "fq_common.h"
#include "fq_shuffle_i8_geom.h"

namespace fq {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <bool LDS>
__global__ __launch_bounds__(kShufBlock) void shuffle_i8_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                const ShufGeom s) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[LDS ? kShufLdsBytes : 16];
    const unsigned char* __restrict__ xb = reinterpret_cast<const unsigned char*>(x);
    const unsigned tid = threadIdx.x;
    for (unsigned t = blockIdx.x; t < s.ntiles; t += gridDim.x) {
        const unsigned pix0 = t * (unsigned)s.TP;
        const unsigned np = shuf_tile_pixels(s, t);
        if constexpr (LDS) {
            const unsigned items = np * (unsigned)s.SU;
            for (unsigned i = tid; i < items; i += kShufBlock)
                *reinterpret_cast<v4u*>(tile + 16u * i) = *reinterpret_cast<const v4u*>(xb + shuf_stage_src(s, pix0, i));
            __syncthreads();
        }
        const unsigned units = np * (unsigned)s.CH;
        for (unsigned o = tid; o < units; o += kShufBlock) {
            const unsigned p = o / (unsigned)s.CH, k = o - p * (unsigned)s.CH;
            const unsigned char* row = (LDS ? tile : xb) + shuf_row_base(s, pix0, p);
            ShufWalk w = shuf_walk_begin(s, k);
            unsigned d[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned v = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (shuf_walk_real(s, w)) v |= (unsigned)row[shuf_walk_rel(s, w)] << (8 * b);
                    shuf_walk_next(s, w);
                }
                d[q] = v;
            }
            v4u out;
            out.x = d[0]; out.y = d[1]; out.z = d[2]; out.w = d[3];
            *reinterpret_cast<v4u*>(y + (size_t)(pix0 + p) * (size_t)s.Cpad_out + 16u * k) = out;
        }
        if constexpr (LDS) __syncthreads();                 // the next tile's stage overwrites what slower lanes still read
    }
}

}  // namespace fq

using namespace fq;

extern "C" int fq_shuffle_i8_nhwc_supported(int C_in, int c_off, int C, int groups) {
    if (C_in < 1 || C < 1 || c_off < 0 || (long)c_off + C > C_in) return 0;
    const int cpad_in = shuf_pad16(C_in);
    if (!shuf_args_ok(cpad_in, c_off, C, groups)) return 0;
    if (groups == 1 && c_off == 0 && cpad_in == shuf_pad16(C)) return 0;          // nothing to do
    return 1;
}

extern "C" int fq_shuffle_i8_nhwc(const int8_t* x, int Cpad_in, int c_off, int8_t* y, int Cpad_out, int C, int groups, int N,
                                  int H, int W, fq_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || Cpad_in < 1) return FQ_ERR_INVALID_ARG;
    if (C < 1 || c_off < 0 || groups < 1 || C % groups != 0) return FQ_ERR_INVALID_ARG;
    if (Cpad_in % 16) return FQ_ERR_UNSUPPORTED;
    if ((long)c_off + C > Cpad_in) return FQ_ERR_INVALID_ARG;
    if (C > kShufMaxC) return FQ_ERR_UNSUPPORTED;
    if (Cpad_out != shuf_pad16(C)) return FQ_ERR_INVALID_ARG;
    if (groups == 1 && c_off == 0 && Cpad_in == Cpad_out) return FQ_ERR_INVALID_ARG;      // nothing to do
    if (N == 0) return FQ_OK;
    if (!x || !y || (reinterpret_cast<uintptr_t>(x) & 15u) || (reinterpret_cast<uintptr_t>(y) & 15u)) return FQ_ERR_INVALID_ARG;
    // 32-bit pixel and element arithmetic in the kernel
    long npix = (long)N * H;
    if (npix >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    npix *= W;
    if (npix >= 0x7fffffffL || npix * Cpad_in >= 0x7fffffffL || npix * Cpad_out >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    const ShufGeom s = shuf_geom(Cpad_in, c_off, C, groups, (unsigned)npix);
    const unsigned blocks = shuf_blocks(s);
    hipStream_t st = as_stream(stream);
    if (s.lds) shuffle_i8_kernel<true><<<blocks, kShufBlock, 0, st>>>(x, y, s);
    else shuffle_i8_kernel<false><<<blocks, kShufBlock, 0, st>>>(x, y, s);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
