// fq_concat_rq_i8.hip -- channel concatenation of resident NHWC activations that lie on DIFFERENT grids, or whose readers quantise
// at another bit than their grid, in ONE launch: every source is re-quantised from its own grid to the readers' bit on the way
// (include/fq.h: fq_concat_rq_i8_nhwc).  A source is int8, or the exact int16 sum of a resident NewAdd; each has its own
// nearest-upsampling factor, ReLU flag and shift = b - g_i.
//
//   base_i = C_0 + ... + C_{i-1},  v = src_i[n][h / up_i][w / up_i][c - base_i]
//   r = rint(v * 2^shift_i)                                        half to even; an exact left shift for shift_i >= 0
//   out[n][h][w][c] = clamp(relu_i ? max(r, 0) : r, -128, 127)     base_i <= c < base_i + C_i
//                   = 0                                            sum C <= c < Cpad_out
//
// The reference's chain DeQuantity_g -> (nearest up) -> cat -> (ReLU) -> Quantity_b scales by powers of two only, so it is this
// integer function with one rounding per element.  Bandwidth-bound: 1 or 2 bytes read and 1 written per output byte; no LDS, no
// inline assembly, vector stores only.  The shape is fq_concat_i8.hip's:
//   * one lane owns one 16-byte chunk of the output (fq_concat_rq_i8_geom.h) and stores it with one dwordx4; lanes run channel
//     fastest; at most 2048 workgroups of 256, a lane keeps its chunk index k and strides over the pixels, so which sources it
//     reads, at which offsets, under which masks, with which shift and ReLU is computed once per lane in front of the pixel loop;
//   * the shift is a RUNTIME value, uniform per source and, in the aligned family, per lane: one code path does the rounding
//     right shift, the identity and the clamped left shift (crq_requant: rsh, lsh, mask, bias, odd, lo), twelve packed-int16
//     instructions per two elements.  Compile-time modes per launch (as fq_upsample_bilinear_i8.hip has) would have to be chosen
//     for the whole launch while the sources of one launch differ in sign of shift -- the case this kernel exists for;
//   * GENERAL == false: every base_i % 16 == 0 (what models hit).  Every chunk is 16 elements of one source at a 16-element
//     offset: one dwordx4 load of an int8 source, two of an int16 source (the branch is per lane: a wave whose lanes own chunks
//     of both kinds runs both loads, the arithmetic behind them is shared), the re-quantisation, the tail mask, the store.
//     The owner's values are picked with a chain of selects over compile-time source indices;
//   * GENERAL == true: a chunk with one owner at a 16-element offset still takes that path; every other chunk is or-ed together
//     from the parts of every source with an element in it.  A part is built from aligned dword loads and v_alignbyte_b32 (five
//     dwords of an int8 source, nine of an int16 source at an odd channel offset), re-quantised with ITS source's shift and ReLU
//     and masked to its own byte range BEFORE the or: a source's padding never reaches the output.  A dword that holds no
//     wanted byte is not loaded (CrqPart::ld), which keeps every load inside the row.  The loop over the sources is unrolled
//     under the uniform guard i < nsrc, so every per-source value sits in registers (no scratch);
//   * UPS == true when a source is upsampled: the pixel is split into (n, h, w) once and source i reads (n, h >> lu, w >> lu).
//     Without it source pixel == output pixel and the loop holds no division.
// Every load is aligned and lies inside its source; scripts/concat_rq_geom_check.cpp walks the same functions on the host.
#include "fq_common.h"
#include "fq_concat_rq_i8_geom.h"

namespace fq {

struct CrqParams {
    CrqGeom g;
    const char* q[kCrqMaxSrc];
};

typedef unsigned crq_v4u __attribute__((ext_vector_type(4)));
typedef short crq_s2 __attribute__((ext_vector_type(2)));

struct CrqRoundPk { crq_s2 rsh, lsh, mask, bias, odd, lo; };

__device__ __forceinline__ crq_s2 crq_dup(int v) { return crq_s2{(short)v, (short)v}; }

__device__ __forceinline__ CrqRoundPk crq_round_pk(int rsh, int lsh, int mask, int bias, int odd, int lo) {
    return CrqRoundPk{crq_dup(rsh), crq_dup(lsh), crq_dup(mask), crq_dup(bias), crq_dup(odd), crq_dup(lo)};
}

// crq_requant (fq_concat_rq_i8_geom.h) on two int16 at once, step for step
__device__ __forceinline__ crq_s2 crq_requant_pk(crq_s2 v, const CrqRoundPk& r) {
    const crq_s2 hi = {127, 127};
    const crq_s2 q = v >> r.rsh;
    const crq_s2 t = ((v & r.mask) + r.bias + (q & r.odd)) >> r.rsh;
    crq_s2 x = q + t;
    x = __builtin_elementwise_min(__builtin_elementwise_max(x, r.lo), hi) << r.lsh;
    return __builtin_elementwise_min(__builtin_elementwise_max(x, r.lo), hi);
}

// Sixteen elements as eight pairs: ev[t] = elements (4t, 4t + 2), od[t] = elements (4t + 1, 4t + 3) -- the order in which two
// re-quantised pairs go back into dword t with two masks, a shift and an or.
struct CrqElems { crq_s2 ev[4], od[4]; };

// four dwords of int8
__device__ __forceinline__ CrqElems crq_unpack8(const unsigned (&d)[4]) {
    CrqElems e;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        e.ev[t] = __builtin_bit_cast(crq_s2, d[t] << 8) >> 8;
        e.od[t] = __builtin_bit_cast(crq_s2, d[t]) >> 8;
    }
    return e;
}

// eight dwords of int16: dword 2t = elements (4t, 4t + 1), dword 2t + 1 = elements (4t + 2, 4t + 3)
__device__ __forceinline__ CrqElems crq_unpack16(const unsigned (&d)[8]) {
    CrqElems e;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        e.ev[t] = __builtin_bit_cast(crq_s2, (d[2 * t] & 0x0000ffffu) | (d[2 * t + 1] << 16));
        e.od[t] = __builtin_bit_cast(crq_s2, (d[2 * t] >> 16) | (d[2 * t + 1] & 0xffff0000u));
    }
    return e;
}

// dword t of the chunk from the re-quantised elements
__device__ __forceinline__ unsigned crq_dword(const CrqElems& e, int t, const CrqRoundPk& r) {
    const unsigned ev = __builtin_bit_cast(unsigned, crq_requant_pk(e.ev[t], r));
    const unsigned od = __builtin_bit_cast(unsigned, crq_requant_pk(e.od[t], r));
    return (ev & 0x00ff00ffu) | ((od & 0x00ff00ffu) << 8);
}

// The chunk k is 16 elements of ONE source at a 16-element-aligned offset of its pixel row.
template <bool UPS>
__device__ __forceinline__ void crq_loop16(int8_t* __restrict__ out, const CrqParams& p, int k, unsigned pix, unsigned stride) {
    const CrqGeom& g = p.g;
    const char* __restrict__ src = p.q[0];
    int off = 0, hi = 16, lu = 0, wide = 0;
    unsigned rowbytes = 16u;
    int rsh = 0, lsh = 0, mask = 0, bias = 0, odd = 0, lo = -128;
#pragma unroll
    for (int i = 0; i < kCrqMaxSrc; ++i) {
        const CrqPart pi = crq_part(g, k, i);
        const bool own = pi.use != 0;
        const int eb = g.s[i].wide ? 2 : 1;
        src = own ? p.q[i] : src;
        off = own ? pi.s * eb : off;
        hi = own ? pi.hi : hi;
        lu = own ? g.s[i].lu : lu;
        wide = own ? g.s[i].wide : wide;
        rowbytes = own ? (unsigned)(g.s[i].Cpad * eb) : rowbytes;
        rsh = own ? g.r[i].rsh : rsh;
        lsh = own ? g.r[i].lsh : lsh;
        mask = own ? g.r[i].mask : mask;
        bias = own ? g.r[i].bias : bias;
        odd = own ? g.r[i].odd : odd;
        lo = own ? g.r[i].lo : lo;
    }
    const CrqRoundPk r = crq_round_pk(rsh, lsh, mask, bias, odd, lo);
    unsigned m[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) m[t] = cat_dword_mask(0, hi, t);
    for (; pix < g.npix; pix += stride) {
        unsigned sp = pix;
        if constexpr (UPS) {
            const unsigned w = pix % (unsigned)g.W, rr = pix / (unsigned)g.W;
            sp = crq_src_pix(g, lu, rr / (unsigned)g.H, rr % (unsigned)g.H, w);
        }
        const char* at = src + (size_t)sp * rowbytes + off;
        CrqElems e;
        if (wide) {
            const crq_v4u d0 = *reinterpret_cast<const crq_v4u*>(at);
            const crq_v4u d1 = *reinterpret_cast<const crq_v4u*>(at + 16);
            const unsigned d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            e = crq_unpack16(d);
        } else {
            const crq_v4u d0 = *reinterpret_cast<const crq_v4u*>(at);
            const unsigned d[4] = {d0.x, d0.y, d0.z, d0.w};
            e = crq_unpack8(d);
        }
        crq_v4u v;
        v.x = crq_dword(e, 0, r) & m[0];
        v.y = crq_dword(e, 1, r) & m[1];
        v.z = crq_dword(e, 2, r) & m[2];
        v.w = crq_dword(e, 3, r) & m[3];
        *reinterpret_cast<crq_v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = v;
    }
}

template <bool GENERAL, bool UPS>
__global__ __launch_bounds__(kCatBlock) void concat_rq_i8_kernel(int8_t* __restrict__ out, const CrqParams p) {
    const CrqGeom& g = p.g;
    const unsigned gid = blockIdx.x * kCatBlock + threadIdx.x;
    const unsigned stride = (gridDim.x * kCatBlock) / (unsigned)g.CH;
    const int k = (int)(gid % (unsigned)g.CH);
    unsigned pix = gid / (unsigned)g.CH;
    if (pix >= stride) return;

    if constexpr (!GENERAL) {
        crq_loop16<UPS>(out, p, k, pix, stride);
    } else {
        int a[kCrqMaxSrc], sh[kCrqMaxSrc];
        unsigned ld[kCrqMaxSrc], m[kCrqMaxSrc][4];
        int owners = 0, whole = 0;
#pragma unroll
        for (int i = 0; i < kCrqMaxSrc; ++i) {
            const CrqPart pi = crq_part(g, k, i);
            owners += pi.use;
            whole |= pi.use & pi.whole16;
            a[i] = pi.a;
            sh[i] = pi.sh;
            ld[i] = pi.ld;                                  // 0 where the source has no element in the chunk
#pragma unroll
            for (int t = 0; t < 4; ++t) m[i][t] = pi.use ? cat_dword_mask(pi.lo, pi.hi, t) : 0u;
        }
        if (owners == 1 && whole) {
            crq_loop16<UPS>(out, p, k, pix, stride);
            return;
        }
        for (; pix < g.npix; pix += stride) {
            unsigned n = 0, h = 0, w = 0;
            if constexpr (UPS) {
                w = pix % (unsigned)g.W;
                const unsigned rr = pix / (unsigned)g.W;
                h = rr % (unsigned)g.H;
                n = rr / (unsigned)g.H;
            }
            unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < kCrqMaxSrc; ++i) {
                if (i < g.nsrc) {                           // uniform
                    if (ld[i]) {
                        const unsigned sp = UPS ? crq_src_pix(g, g.s[i].lu, n, h, w) : pix;
                        const CrqRoundPk r = crq_round_pk(g.r[i].rsh, g.r[i].lsh, g.r[i].mask, g.r[i].bias, g.r[i].odd, g.r[i].lo);
                        CrqElems e;
                        if (g.s[i].wide) {                  // uniform
                            const char* row = p.q[i] + (size_t)sp * (unsigned)(2 * g.s[i].Cpad);
                            unsigned d[9], c[8];
#pragma unroll
                            for (int t = 0; t < 9; ++t) {
                                d[t] = 0u;
                                if (ld[i] & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (a[i] + 4 * t));
                            }
#pragma unroll
                            for (int t = 0; t < 8; ++t) c[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)sh[i]);
                            e = crq_unpack16(c);
                        } else {
                            const char* row = p.q[i] + (size_t)sp * (unsigned)g.s[i].Cpad;
                            unsigned d[5], c[4];
#pragma unroll
                            for (int t = 0; t < 5; ++t) {
                                d[t] = 0u;
                                if (ld[i] & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (a[i] + 4 * t));
                            }
#pragma unroll
                            for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)sh[i]);
                            e = crq_unpack8(c);
                        }
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] |= crq_dword(e, t, r) & m[i][t];
                    }
                }
            }
            crq_v4u o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<crq_v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = o;
        }
    }
}

}  // namespace fq

using namespace fq;

extern "C" int fq_concat_rq_i8_nhwc_supported(const int* C, const int* up, const int* bytes, const int* shift, int nsrc) {
    return crq_supported(C, up, bytes, shift, nsrc) ? 1 : 0;
}

extern "C" int fq_concat_rq_i8_nhwc(const fq_cat_src_rq* srcs, int nsrc, int8_t* out, int Cpad_out, int N, int H, int W,
                                    fq_stream_t stream) {
    if (!srcs) return FQ_ERR_INVALID_ARG;
    int bytes[kCrqMaxSrc], C[kCrqMaxSrc], Cpad[kCrqMaxSrc], up[kCrqMaxSrc], relu[kCrqMaxSrc], shift[kCrqMaxSrc];
    for (int i = 0; i < nsrc && i < kCrqMaxSrc; ++i) {
        bytes[i] = srcs[i].bytes; C[i] = srcs[i].C; Cpad[i] = srcs[i].Cpad; up[i] = srcs[i].up; relu[i] = srcs[i].relu;
        shift[i] = srcs[i].shift;
    }
    const int rc = crq_args(bytes, C, Cpad, up, relu, shift, nsrc, Cpad_out, N, H, W);
    if (rc) return rc == -1 ? FQ_ERR_INVALID_ARG : FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return FQ_ERR_INVALID_ARG;
    for (int i = 0; i < nsrc; ++i)
        if (!srcs[i].q || (reinterpret_cast<uintptr_t>(srcs[i].q) & 15u)) return FQ_ERR_INVALID_ARG;
    CrqParams p;
    p.g = crq_geom(bytes, C, Cpad, up, relu, shift, nsrc, Cpad_out, N, H, W);
    for (int i = 0; i < kCrqMaxSrc; ++i) p.q[i] = static_cast<const char*>(srcs[i < nsrc ? i : 0].q);
    const bool general = !crq_aligned(p.g), ups = crq_upsampled(p.g);
    const unsigned blocks = (unsigned)crq_blocks(p.g);
    hipStream_t st = as_stream(stream);
    if (general) {
        if (ups) concat_rq_i8_kernel<true, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_rq_i8_kernel<true, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    } else {
        if (ups) concat_rq_i8_kernel<false, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_rq_i8_kernel<false, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
