// fq_act_lut_i8.hip -- an elementwise activation between two integer layers as a 256-entry table on resident int8 NHWC
// activations (include/fq.h: fq_act_lut_i8_nhwc).
//
//   y[n][h][w][c] = table[x[n][h][w][c] + 128]     0 <= c < C
//                 = 0                               C <= c < Cpad, whatever the table holds
//
// The table is Quantity_b(f(DeQuantity_g(q))) for the 256 values of q, made by the caller with the library's own elementwise ops
// (common/quantity/_native.py: build_act_table), so the kernel has no arithmetic of its own: one byte in, one byte out.
//   * a lane moves 16 bytes per load and per store (dwordx4); the tensor is one run of bytes, cut into 16-byte chunks
//     (fq_act_lut_i8_geom.h), at most 2048 workgroups stride over them; every lane of a workgroup makes the same number of
//     passes, a lane past the last chunk neither loads nor stores;
//   * two forms of the lookup, both kept (kActLutForm names the one the entry point runs; fq_debug_act_lut_i8_form runs either,
//     for scripts/activation_cost.py):
//       form 0: the 256 bytes staged once per workgroup in LDS, one byte read per element.  A sub-dword read banks by (a / 4) mod 32,
//               so the 64 table dwords lie two to a bank and lanes that hit different dwords of one bank serialise;
//       form 1: the table held in registers, dword l in lane l of every wave, fetched with ds_bpermute_b32 (the LDS crossbar
//               without the LDS array: no banks) and the byte picked with a shift;
//   * padding channels are masked to zero after the lookup (act_lut_real_mask): f(0) != 0 for a Sigmoid, and every consumer
//     relies on zero padding;
//   * the n % 16 bytes behind the last chunk (only where Cpad is no multiple of 16) are taken one byte per lane by workgroup 0,
//     reading the table from global memory.
// Every access lies inside [x, x + n), [y, y + n) and [table, table + 256); scripts/act_lut_geom_check.cpp walks the same
// functions on the host over the tests' shapes.
#include "fq_common.h"
#include "fq_act_lut_i8_geom.h"

namespace fq {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int kActLutForm = 0;       // measured: profiles/r17_activation_lut.txt

template <int FORM>
__global__ __launch_bounds__(kActLutBlock) void act_lut_i8_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                  const int8_t* __restrict__ table, const ActLutGeom g) {
    __shared__ unsigned char lut[FORM == 0 ? 256 : 4];
    const unsigned char* __restrict__ tb = reinterpret_cast<const unsigned char*>(table);
    const unsigned tid = threadIdx.x;
    unsigned mine = 0u;                                      // form 1: table dword (tid mod 64)
    if constexpr (FORM == 0) {
        lut[tid] = tb[tid];
        __syncthreads();
    } else {
        const unsigned l = (tid & 63u) * 4u;
        mine = (unsigned)tb[l] | ((unsigned)tb[l + 1u] << 8) | ((unsigned)tb[l + 2u] << 16) | ((unsigned)tb[l + 3u] << 24);
    }
    for (unsigned p = 0; p < g.passes; ++p) {
        const unsigned long long chunk = act_lut_chunk(g, blockIdx.x, tid, p);
        const bool active = chunk < (unsigned long long)g.chunks;
        const unsigned o = active ? (unsigned)chunk * 16u : 0u;
        v4u in = {0u, 0u, 0u, 0u};
        if (active) in = *reinterpret_cast<const v4u*>(x + o);
        const unsigned w[4] = {in.x ^ 0x80808080u, in.y ^ 0x80808080u, in.z ^ 0x80808080u, in.w ^ 0x80808080u};    // q + 128
        unsigned d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned v = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned idx = (w[q] >> (8 * b)) & 0xffu;
                unsigned t;
                if constexpr (FORM == 0) {
                    t = lut[idx];
                } else {                                     // (all lanes of the wave take part: outside `if (active)`)
                    const unsigned dw = (unsigned)__builtin_amdgcn_ds_bpermute((int)(idx & ~3u), (int)mine);
                    t = (dw >> ((idx & 3u) * 8u)) & 0xffu;
                }
                v |= t << (8 * b);
            }
            d[q] = v;
        }
        if (active) {
            const unsigned m = act_lut_real_mask(g, o);
            v4u out;
            out.x = d[0] & act_lut_byte_mask(m & 15u);
            out.y = d[1] & act_lut_byte_mask((m >> 4) & 15u);
            out.z = d[2] & act_lut_byte_mask((m >> 8) & 15u);
            out.w = d[3] & act_lut_byte_mask((m >> 12) & 15u);
            *reinterpret_cast<v4u*>(y + o) = out;
        }
    }
    if (blockIdx.x == 0 && tid < g.tail) {
        const unsigned o = act_lut_tail_offset(g, tid);
        y[o] = act_lut_tail_real(g, tid) ? table[(unsigned)(x[o] + 128)] : (int8_t)0;
    }
}

static int act_lut_launch(const int8_t* x, int8_t* y, const int8_t* table, int N, int H, int W, int C, int Cpad, int form,
                          fq_stream_t stream) {
    if (!x || !y || !table) return FQ_ERR_INVALID_ARG;
    const int rc = act_lut_args(N, H, W, C, Cpad);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(x) & 15u) || (reinterpret_cast<uintptr_t>(y) & 15u)) return FQ_ERR_INVALID_ARG;
    const ActLutGeom g = act_lut_geom((unsigned)((long)N * H * W), C, Cpad);
    hipStream_t st = as_stream(stream);
    if (form == 0) act_lut_i8_kernel<0><<<g.blocks, kActLutBlock, 0, st>>>(x, y, table, g);
    else act_lut_i8_kernel<1><<<g.blocks, kActLutBlock, 0, st>>>(x, y, table, g);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_act_lut_i8_nhwc_supported(int C) { return C >= 1 ? 1 : 0; }

extern "C" int fq_act_lut_i8_nhwc(const int8_t* x, int8_t* y, const int8_t* table256, int N, int H, int W, int C, int Cpad,
                                  fq_stream_t stream) {
    return act_lut_launch(x, y, table256, N, H, W, C, Cpad, kActLutForm, stream);
}

// Either form of the lookup on the same arguments (form 0 / 1 above), for the launch-by-launch timing of
// scripts/activation_cost.py.  Not part of the ABI of include/fq.h.
extern "C" int fq_debug_act_lut_i8_form(const int8_t* x, int8_t* y, const int8_t* table256, int N, int H, int W, int C, int Cpad,
                                        int form, fq_stream_t stream) {
    if (form != 0 && form != 1) return FQ_ERR_INVALID_ARG;
    return act_lut_launch(x, y, table256, N, H, W, C, Cpad, form, stream);
}
