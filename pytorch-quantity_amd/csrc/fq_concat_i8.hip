// fq_concat_i8.hip -- channel concatenation and nearest upsampling of resident NHWC activations in ONE launch, each source with its
// own nearest-upsampling factor and its own ReLU (include/fq.h).  One kernel skeleton, two element policies:
//
//   base_i = C_0 + ... + C_{i-1},  v = src_i[n][h / up_i][w / up_i][c - base_i]
//   out[n][h][w][c] = f_i(v)     base_i <= c < base_i + C_i
//                   = 0          sum C <= c < Cpad_out
//   CatMove (fq_concat_i8_nhwc for one or two sources, fq_concat_n_i8_nhwc for up to eight): int8 sources on the SAME grid g (the
//     calibrator's merge group gives a Concat's operands one bit), so moving the integers is concatenating the values;
//     f_i = max(., 0) where relu_i == 1, else the identity.  What nested Concat markers compute, without the intermediate tensors:
//     three nested two-source launches over branch widths a, b, c, d move 2(a+b) + 2(a+b+c) + 2(a+b+c+d) bytes per pixel, one
//     launch 2(a+b+c+d).
//   CatRequant (fq_concat_rq_i8_nhwc): sources on DIFFERENT grids, or whose readers quantise at another bit than their grid; a
//     source is int8, or the exact int16 sum of a resident NewAdd, and is re-quantised on the way with shift_i = b - g_i:
//     f_i(v) = clamp(relu_i ? max(r, 0) : r, -128, 127), r = rint(v * 2^shift_i), half to even, an exact left shift for shift_i >= 0.
//     The reference's chain DeQuantity_g -> (nearest up) -> cat -> (ReLU) -> Quantity_b scales by powers of two only, so it is this
//     integer function with one rounding per element.
//
// Bandwidth-bound: HBM is the only resource; no LDS, no inline assembly, vector stores only.
// The skeleton, concat_kernel<ELEM, MAXSRC, GENERAL, UPS> (ELEM = CatMove at MAXSRC = 2 and 8, CatRequant at 8: the two-source launch
// keeps a parameter block of two entries and 8 waves per SIMD in every family, which the eight-entry general family does not reach):
//   * one lane owns one 16-byte chunk of the output (fq_concat_i8_geom.h) and stores it with one dwordx4; lanes run channel
//     fastest, so a wave stores whole contiguous pixels; at most 2048 workgroups of 256, a lane keeps its chunk index k and
//     strides over the pixels, so which sources it reads, at which offsets, under which masks, with which ELEM arguments is
//     computed once per lane in front of the pixel loop;
//   * GENERAL == false: every base_i % 16 == 0 (what models hit: branch widths in multiples of 16; every single-source call).
//     Every chunk is 16 elements of one source at a 16-element-aligned offset: ELEM's 16-element load, its transform, the tail
//     mask, the store.  The owner's pointer, row size, offset, factor and ELEM arguments are picked with a chain of selects over
//     compile-time source indices -- indexing the kernel arguments with a per-lane index would turn them into vector loads of
//     the argument block;
//   * GENERAL == true: a chunk with one owner at a 16-element-aligned source offset still takes that path; every other chunk is
//     or-ed together from the parts of every source with an element in it.  A part is built from aligned dword loads and
//     v_alignbyte_b32 (a runtime byte shift of a 64-bit pair; cat_gather), passed through ELEM's transform with ITS source's
//     arguments and masked to its own byte range BEFORE the or: a source's padding never reaches the output.  A dword that
//     holds no wanted byte is not loaded (CatPart::ld), which is also what keeps the last dword of a row's last chunk inside the
//     row.  The loop over the sources is unrolled under the uniform guard i < nsrc, so every per-source value sits in registers
//     (no scratch);
//   * UPS == true when a source is upsampled: the pixel is split into (n, h, w) once and source i reads (n, h >> lu_i, w >> lu_i);
//     neighbouring output pixels re-read the same source pixel from L1 / L2.  Without it source pixel == output pixel and the
//     loop holds no division.
// An element policy owns what depends on the element: its per-source kernel arguments (Src; the parameter block holds MAXSRC of
// them and nothing of the other policy; none / pick are its links of the owner-select chain), those arguments made ready for the
// pixel loop (Own), the element size, the 16-element load and the transform of assembled dwords into the chunk's dwords.
//   * CatMove: Src is the ReLU's sign mask; one dwordx4 load, five dwords in the general family; the mask, then relu4;
//   * CatRequant: Src is `wide` and the CrqRound; one dwordx4 load of an int8 source, two of an int16 source (the branch is per
//     lane in the aligned family: a wave whose lanes own chunks of both kinds runs both loads, the arithmetic behind them is
//     shared), five or nine dwords in the general family; unpack to packed int16, crq_requant_pk, repack, then the mask.  The
//     shift is a RUNTIME value, uniform per source and, in the aligned family, per lane: one code path does the rounding right
//     shift, the identity and the clamped left shift (crq_requant: rsh, lsh, mask, bias, odd, lo), twelve packed-int16
//     instructions per two elements.  Compile-time modes per launch (as fq_upsample_bilinear_i8.hip has) would have to be chosen
//     for the whole launch while the sources of one launch differ in sign of shift -- the case this policy exists for.
// Every load is aligned and lies inside [q_i, q_i + N (H / up_i) (W / up_i) Cpad_i bytes_i); scripts/concat_geom_check.cpp walks
// the same functions on the host over the tests' shapes, for both policies and at both source limits.
#include "fq_common.h"
#include "fq_concat_i8_geom.h"

namespace fq {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef short crq_s2 __attribute__((ext_vector_type(2)));

template <class ELEM, int MAXSRC>
struct CatParams {
    CatGeom<MAXSRC> g;
    const char* q[MAXSRC];
    typename ELEM::Src e[MAXSRC];
};

// The general family's loads: ND dwords of a part's elements from ND + 1 aligned dwords at row + a, shifted down by sh bytes.
template <int ND>
__device__ __forceinline__ void cat_gather(const char* row, int a, int sh, unsigned ld, unsigned (&c)[ND]) {
    unsigned d[ND + 1];
#pragma unroll
    for (int t = 0; t < ND + 1; ++t) {
        d[t] = 0u;
        if (ld & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (a + 4 * t));
    }
#pragma unroll
    for (int t = 0; t < ND; ++t) c[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)sh);
}

// ---------------------------------------------------------------- the moving policy
struct CatMove {
    struct Src { unsigned relu_sign; };                    // 0x80808080 where the source passes through a ReLU, else 0
    typedef Src Own;
    static Src src(int, int relu, int) { return Src{relu ? 0x80808080u : 0u}; }
    __device__ __forceinline__ static int bytes(const Src&) { return 1; }
    __device__ __forceinline__ static Src none() { return Src{0u}; }
    __device__ __forceinline__ static Src pick(bool own, const Src& s, const Src& o) { return Src{own ? s.relu_sign : o.relu_sign}; }
    __device__ __forceinline__ static Own ready(const Src& s) { return s; }

    // max(byte, 0) on four int8 at once where sign = 0x80808080; the identity where sign = 0
    __device__ __forceinline__ static unsigned relu4(unsigned x, unsigned sign) { return x & ~(((x & sign) >> 7) * 0xffu); }

    // v = the 16 elements at `at` under the masks m
    __device__ __forceinline__ static void chunk16(const char* at, const Own& o, const unsigned (&m)[4], unsigned (&v)[4]) {
        const v4u d = *reinterpret_cast<const v4u*>(at);
        v[0] = relu4(d.x & m[0], o.relu_sign);
        v[1] = relu4(d.y & m[1], o.relu_sign);
        v[2] = relu4(d.z & m[2], o.relu_sign);
        v[3] = relu4(d.w & m[3], o.relu_sign);
    }

    // v = the part of a source whose row starts at `row`, under the masks m (the skeleton ors the parts together)
    __device__ __forceinline__ static void part(const char* row, int a, int sh, unsigned ld, const Own& o, const unsigned (&m)[4],
                                                unsigned (&v)[4]) {
        unsigned c[4];
        cat_gather<4>(row, a, sh, ld, c);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = relu4(c[t] & m[t], o.relu_sign);
    }
};

// ---------------------------------------------------------------- the re-quantising policy
struct CrqRoundPk { crq_s2 rsh, lsh, mask, bias, odd, lo; };

__device__ __forceinline__ crq_s2 crq_dup(int v) { return crq_s2{(short)v, (short)v}; }

// crq_requant (fq_concat_i8_geom.h) on two int16 at once, step for step
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

struct CatRequant {
    struct Src { int wide; CrqRound r; };                  // wide: 1 int16 elements, 0 int8
    struct Own { int wide; CrqRoundPk r; };
    static Src src(int bytes, int relu, int shift) { return Src{bytes == 2 ? 1 : 0, crq_round(shift, relu)}; }
    __device__ __forceinline__ static int bytes(const Src& s) { return s.wide ? 2 : 1; }
    __device__ __forceinline__ static Src none() { return Src{0, CrqRound{0, 0, 0, 0, 0, -128}}; }
    __device__ __forceinline__ static Src pick(bool own, const Src& s, const Src& o) {
        return Src{own ? s.wide : o.wide, CrqRound{own ? s.r.rsh : o.r.rsh, own ? s.r.lsh : o.r.lsh, own ? s.r.mask : o.r.mask,
                                                    own ? s.r.bias : o.r.bias, own ? s.r.odd : o.r.odd, own ? s.r.lo : o.r.lo}};
    }
    __device__ __forceinline__ static Own ready(const Src& s) {
        return Own{s.wide, CrqRoundPk{crq_dup(s.r.rsh), crq_dup(s.r.lsh), crq_dup(s.r.mask), crq_dup(s.r.bias), crq_dup(s.r.odd), crq_dup(s.r.lo)}};
    }

    __device__ __forceinline__ static void chunk16(const char* at, const Own& o, const unsigned (&m)[4], unsigned (&v)[4]) {
        CrqElems e;
        if (o.wide) {
            const v4u d0 = *reinterpret_cast<const v4u*>(at);
            const v4u d1 = *reinterpret_cast<const v4u*>(at + 16);
            const unsigned d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            e = crq_unpack16(d);
        } else {
            const v4u d0 = *reinterpret_cast<const v4u*>(at);
            const unsigned d[4] = {d0.x, d0.y, d0.z, d0.w};
            e = crq_unpack8(d);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = crq_dword(e, t, o.r) & m[t];
    }

    __device__ __forceinline__ static void part(const char* row, int a, int sh, unsigned ld, const Own& o, const unsigned (&m)[4],
                                                unsigned (&v)[4]) {
        CrqElems e;
        if (o.wide) {                                       // uniform
            unsigned c[8];
            cat_gather<8>(row, a, sh, ld, c);
            e = crq_unpack16(c);
        } else {
            unsigned c[4];
            cat_gather<4>(row, a, sh, ld, c);
            e = crq_unpack8(c);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = crq_dword(e, t, o.r) & m[t];
    }
};

// ---------------------------------------------------------------- the skeleton
// The chunk k is 16 elements of ONE source at a 16-element-aligned offset of its pixel row.
template <class ELEM, int MAXSRC, bool UPS>
__device__ __forceinline__ void cat_loop16(int8_t* __restrict__ out, const CatParams<ELEM, MAXSRC>& p, int k, unsigned pix, unsigned stride) {
    const CatGeom<MAXSRC>& g = p.g;
    const char* __restrict__ src = p.q[0];
    int off = 0, hi = 16, lu = 0;
    unsigned rowbytes = 16u;
    typename ELEM::Src sel = ELEM::none();
#pragma unroll
    for (int i = 0; i < MAXSRC; ++i) {
        const int eb = ELEM::bytes(p.e[i]);
        const CatPart pi = cat_part(g, k, i, eb);
        const bool own = pi.use != 0;
        src = own ? p.q[i] : src;
        off = own ? pi.s * eb : off;
        hi = own ? pi.hi : hi;
        lu = own ? g.s[i].lu : lu;
        rowbytes = own ? (unsigned)(g.s[i].Cpad * eb) : rowbytes;
        sel = ELEM::pick(own, p.e[i], sel);
    }
    const typename ELEM::Own o = ELEM::ready(sel);
    unsigned m[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) m[t] = cat_dword_mask(0, hi, t);
    for (; pix < g.npix; pix += stride) {
        unsigned sp = pix;
        if constexpr (UPS) {
            const unsigned w = pix % (unsigned)g.W, r = pix / (unsigned)g.W;
            sp = cat_src_pix(g, lu, r / (unsigned)g.H, r % (unsigned)g.H, w);
        }
        unsigned v[4];
        ELEM::chunk16(src + (size_t)sp * rowbytes + off, o, m, v);
        v4u x;
        x.x = v[0]; x.y = v[1]; x.z = v[2]; x.w = v[3];
        *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = x;
    }
}

template <class ELEM, int MAXSRC, bool GENERAL, bool UPS>
__global__ __launch_bounds__(kCatBlock) void concat_kernel(int8_t* __restrict__ out, const CatParams<ELEM, MAXSRC> p) {
    const CatGeom<MAXSRC>& g = p.g;
    const unsigned gid = blockIdx.x * kCatBlock + threadIdx.x;
    const unsigned stride = (gridDim.x * kCatBlock) / (unsigned)g.CH;
    const int k = (int)(gid % (unsigned)g.CH);
    unsigned pix = gid / (unsigned)g.CH;
    if (pix >= stride) return;

    if constexpr (!GENERAL) {
        cat_loop16<ELEM, MAXSRC, UPS>(out, p, k, pix, stride);
    } else {
        int a[MAXSRC], sh[MAXSRC];
        unsigned ld[MAXSRC], m[MAXSRC][4];
        int owners = 0, whole = 0;
#pragma unroll
        for (int i = 0; i < MAXSRC; ++i) {
            const CatPart pi = cat_part(g, k, i, ELEM::bytes(p.e[i]));
            owners += pi.use;
            whole |= pi.use & pi.whole16;
            a[i] = pi.a;
            sh[i] = pi.sh;
            ld[i] = pi.ld;                                  // 0 where the source has no element in the chunk
#pragma unroll
            for (int t = 0; t < 4; ++t) m[i][t] = pi.use ? cat_dword_mask(pi.lo, pi.hi, t) : 0u;
        }
        if (owners == 1 && whole) {
            cat_loop16<ELEM, MAXSRC, UPS>(out, p, k, pix, stride);
            return;
        }
        for (; pix < g.npix; pix += stride) {
            unsigned n = 0, h = 0, w = 0;
            if constexpr (UPS) {
                w = pix % (unsigned)g.W;
                const unsigned r = pix / (unsigned)g.W;
                h = r % (unsigned)g.H;
                n = r / (unsigned)g.H;
            }
            unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < MAXSRC; ++i) {
                if (i < g.nsrc) {                           // uniform
                    if (ld[i]) {
                        const unsigned sp = UPS ? cat_src_pix(g, g.s[i].lu, n, h, w) : pix;
                        const char* row = p.q[i] + (size_t)sp * (unsigned)(g.s[i].Cpad * ELEM::bytes(p.e[i]));
                        unsigned x[4];
                        ELEM::part(row, a[i], sh[i], ld[i], ELEM::ready(p.e[i]), m[i], x);
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] |= x[t];
                    }
                }
            }
            v4u o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = o;
        }
    }
}

// ---------------------------------------------------------------- the entry points
// one source of each entry point's struct as (bytes, relu, shift); the two-source entry point has one ReLU flag for the whole call
static void src_fields(const fq_cat_src&, int relu, int& by, int& rl, int& sf) { by = 1; rl = relu ? 1 : 0; sf = 0; }
static void src_fields(const fq_cat_src_n& s, int, int& by, int& rl, int& sf) { by = 1; rl = s.relu; sf = 0; }
static void src_fields(const fq_cat_src_rq& s, int, int& by, int& rl, int& sf) { by = s.bytes; rl = s.relu; sf = s.shift; }

// Validation and launch of every entry point.  ELEM = CatMove: SRC = fq_cat_src with the call's `relu`, or fq_cat_src_n, and the
// pointers are judged in front of the sizes; ELEM = CatRequant: SRC = fq_cat_src_rq, and the scalars are judged before the pointers.
template <class ELEM, int MAXSRC, class SRC>
static int cat_run(const SRC* srcs, int nsrc, int8_t* out, int Cpad_out, int relu, int N, int H, int W, fq_stream_t stream) {
    constexpr bool kMove = std::is_same<ELEM, CatMove>::value;
    if (!srcs) return FQ_ERR_INVALID_ARG;
    int bytes[MAXSRC], C[MAXSRC], Cpad[MAXSRC], up[MAXSRC], rl[MAXSRC], shift[MAXSRC];
    bool bad_ptrs = !out || (reinterpret_cast<uintptr_t>(out) & 15u);
    for (int i = 0; i < nsrc && i < MAXSRC; ++i) {
        C[i] = srcs[i].C; Cpad[i] = srcs[i].Cpad; up[i] = srcs[i].up;
        src_fields(srcs[i], relu, bytes[i], rl[i], shift[i]);
        bad_ptrs = bad_ptrs || !srcs[i].q || (reinterpret_cast<uintptr_t>(srcs[i].q) & 15u);
    }
    const int rc = cat_args(kMove ? nullptr : bytes, C, Cpad, up, rl, kMove ? nullptr : shift, nsrc, MAXSRC, Cpad_out, N, H, W,
                            kMove && bad_ptrs);
    if (rc) return rc == -1 ? FQ_ERR_INVALID_ARG : FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    if (bad_ptrs) return FQ_ERR_INVALID_ARG;
    CatParams<ELEM, MAXSRC> p;
    p.g = cat_geom<MAXSRC>(C, Cpad, up, nsrc, Cpad_out, N, H, W);
    for (int i = 0; i < MAXSRC; ++i) {
        const bool have = i < nsrc;
        p.q[i] = static_cast<const char*>(static_cast<const void*>(srcs[have ? i : 0].q));
        p.e[i] = ELEM::src(have ? bytes[i] : 1, have ? rl[i] : 0, have ? shift[i] : 0);
    }
    const bool general = !cat_aligned(p.g), ups = cat_upsampled(p.g);
    const unsigned blocks = (unsigned)cat_blocks(p.g);
    hipStream_t st = as_stream(stream);
    if (general) {
        if (ups) concat_kernel<ELEM, MAXSRC, true, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_kernel<ELEM, MAXSRC, true, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    } else {
        if (ups) concat_kernel<ELEM, MAXSRC, false, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_kernel<ELEM, MAXSRC, false, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_concat_i8_nhwc_supported(const int* C, const int* up, int nsrc) {
    return cat_supported(C, up, nullptr, nullptr, nsrc, 2) ? 1 : 0;
}
extern "C" int fq_concat_n_i8_nhwc_supported(const int* C, const int* up, int nsrc) {
    return cat_supported(C, up, nullptr, nullptr, nsrc, FQ_CONCAT_N_MAX_SRC) ? 1 : 0;
}
extern "C" int fq_concat_rq_i8_nhwc_supported(const int* C, const int* up, const int* bytes, const int* shift, int nsrc) {
    return bytes && shift && cat_supported(C, up, bytes, shift, nsrc, kCrqMaxSrc) ? 1 : 0;
}

extern "C" int fq_concat_i8_nhwc(const fq_cat_src* srcs, int nsrc, int8_t* out, int Cpad_out, int relu, int N, int H, int W,
                                 fq_stream_t stream) {
    return cat_run<CatMove, 2>(srcs, nsrc, out, Cpad_out, relu, N, H, W, stream);
}

extern "C" int fq_concat_n_i8_nhwc(const fq_cat_src_n* srcs, int nsrc, int8_t* out, int Cpad_out, int N, int H, int W,
                                   fq_stream_t stream) {
    return cat_run<CatMove, FQ_CONCAT_N_MAX_SRC>(srcs, nsrc, out, Cpad_out, 0, N, H, W, stream);
}

extern "C" int fq_concat_rq_i8_nhwc(const fq_cat_src_rq* srcs, int nsrc, int8_t* out, int Cpad_out, int N, int H, int W,
                                    fq_stream_t stream) {
    return cat_run<CatRequant, kCrqMaxSrc>(srcs, nsrc, out, Cpad_out, 0, N, H, W, stream);
}
