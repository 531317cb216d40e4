// fq_pixel_shuffle_i8.hip -- nn.PixelShuffle(r) / nn.PixelUnshuffle(r) (depth-to-space, space-to-depth) of resident int8 NHWC
// activations (include/fq.h: fq_pixel_shuffle_i8_nhwc).
//
//   inverse == 0:  y[n][h r + i][w r + j][c] = x[n][h][w][c r^2 + i r + j]       0 <= c < C, padding channels zero
//   inverse == 1:  y[n][h][w][c r^2 + i r + j] = x[n][h r + i][w r + j][c]
//
// A permutation of the integers is the same permutation of the values q * 2^-grid: no arithmetic, one byte read and one written
// per element.  The gather has a stride of r^2 bytes that r fixes, so nothing is assembled byte by byte where the shape allows:
//   * aligned family (r in {2, 4}, C % 16 == 0; fq_pixel_shuffle_i8_geom.h): a lane takes the 16 r^2 consecutive bytes of one
//     low-resolution pixel that hold 16 channels at all r^2 positions, as r^2 dwordx4 loads, transposes 4 x 4 byte blocks in
//     registers with v_perm_b32 (eight per block) and stores r^2 dwordx4, one per position.  Lanes run over the chunk index
//     first, so a wave's stores cover whole C-byte pixels of the output row.  The inverse direction is the same with loads and
//     stores exchanged.  No LDS, no byte loop.
//   * general family (r == 3, or C % 16 != 0): a lane builds one 16-byte chunk of the output in memory order (a wave stores
//     1 KiB contiguously); every byte below the real width is taken from the aligned dword of the source that holds it, a
//     byte at or above it is zero without a read, so the source's padding channels never reach the output.
//   * at most 2048 workgroups of 256; a lane strides over the remaining items, its (row, column, chunk) digits advanced by
//     additions and two carries (ps_walk_step): no division in the loop but by the template constant R.
// Every load is an aligned dwordx4 or dword inside [x, x + bytes of x), every store an aligned dwordx4 inside y:
// scripts/pixel_shuffle_geom_check.cpp walks the same functions lane by lane on the host.
#include "fq_common.h"
#include "fq_pixel_shuffle_i8_geom.h"

namespace fq {

static_assert(kPsOk == FQ_OK && kPsInvalid == FQ_ERR_INVALID_ARG && kPsUnsupported == FQ_ERR_UNSUPPORTED, "the guard speaks fq.h's codes");

typedef unsigned ps_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ PsV4 ps_load16(const int8_t* p) {
    const ps_v4u t = *reinterpret_cast<const ps_v4u*>(p);
    PsV4 v;
    v.d[0] = t.x; v.d[1] = t.y; v.d[2] = t.z; v.d[3] = t.w;
    return v;
}

__device__ __forceinline__ void ps_store16(int8_t* p, const PsV4& v) {
    ps_v4u t;
    t.x = v.d[0]; t.y = v.d[1]; t.z = v.d[2]; t.w = v.d[3];
    *reinterpret_cast<ps_v4u*>(p) = t;
}

template <int R, bool INV>
__global__ __launch_bounds__(kPsBlock) void pixel_shuffle_aligned_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                         const PsGeom g) {
    constexpr int Q = R * R;
    unsigned item = blockIdx.x * (unsigned)kPsBlock + threadIdx.x;
    if (item >= g.items) return;
    PsWalk s = ps_walk_begin(g, item);
    for (; item < g.items; item += g.stride) {
        PsV4 in[Q], out[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q)
            in[q] = ps_load16(x + (INV ? ps_shallow_off(g, s, q / R, q % R, R) : ps_deep_off(g, item, q, R)));
        if constexpr (R == 4) ps_net4(in, out);
        else if constexpr (INV) ps_net2_s2d(in, out);
        else ps_net2_d2s(in, out);
#pragma unroll
        for (int q = 0; q < Q; ++q)
            ps_store16(y + (INV ? ps_deep_off(g, item, q, R) : ps_shallow_off(g, s, q / R, q % R, R)), out[q]);
        ps_walk_step(g, s);
    }
}

template <int R>
__global__ __launch_bounds__(kPsBlock) void pixel_shuffle_general_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                         const PsGeom g) {
    unsigned item = blockIdx.x * (unsigned)kPsBlock + threadIdx.x;
    if (item >= g.items) return;
    PsWalk s = ps_walk_begin(g, item);
    for (; item < g.items; item += g.stride) {
        PsV4 out;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            unsigned v = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 4 * m + e;
                if (ps_gen_real(g, s, b)) {
                    const size_t src = ps_gen_src(g, s, b, R);
                    const unsigned word = *reinterpret_cast<const unsigned*>(x + (src & ~(size_t)3));
                    v |= ((word >> (8u * (unsigned)(src & 3u))) & 0xffu) << (8 * e);
                }
            }
            out.d[m] = v;
        }
        ps_store16(y + 16u * (size_t)item, out);
        ps_walk_step(g, s);
    }
}

template <int R>
static void launch_aligned(const int8_t* x, int8_t* y, const PsGeom& g, hipStream_t st) {
    if (g.inverse) pixel_shuffle_aligned_kernel<R, true><<<g.blocks, kPsBlock, 0, st>>>(x, y, g);
    else pixel_shuffle_aligned_kernel<R, false><<<g.blocks, kPsBlock, 0, st>>>(x, y, g);
}

}  // namespace fq

using namespace fq;

extern "C" int fq_pixel_shuffle_i8_nhwc_supported(int C, int r, int inverse) { return ps_family(C, r, inverse) != 0; }

extern "C" int fq_pixel_shuffle_i8_nhwc_family(int C, int r, int inverse) { return ps_family(C, r, inverse); }

extern "C" int fq_pixel_shuffle_i8_nhwc(const int8_t* x, int Cpad_in, int8_t* y, int Cpad_out, int C, int r, int inverse, int N,
                                        int H, int W, fq_stream_t stream) {
    int launch = 0;
    const int rc = ps_guard(reinterpret_cast<uintptr_t>(x), Cpad_in, reinterpret_cast<uintptr_t>(y), Cpad_out, C, r, inverse, N, H, W,
                            &launch);
    if (rc != FQ_OK || !launch) return rc;
    const PsGeom g = ps_geom(C, r, inverse, N, H, W);
    hipStream_t st = as_stream(stream);
    if (g.family == kPsAligned) {
        if (r == 2) launch_aligned<2>(x, y, g, st);
        else launch_aligned<4>(x, y, g, st);
    } else if (r == 2) {
        pixel_shuffle_general_kernel<2><<<g.blocks, kPsBlock, 0, st>>>(x, y, g);
    } else if (r == 3) {
        pixel_shuffle_general_kernel<3><<<g.blocks, kPsBlock, 0, st>>>(x, y, g);
    } else {
        pixel_shuffle_general_kernel<4><<<g.blocks, kPsBlock, 0, st>>>(x, y, g);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
