// fq_concat_i8.hip -- channel concatenation and nearest upsampling of resident int8 NHWC activations in ONE launch, each source
// with its own nearest-upsampling factor and its own ReLU (include/fq.h: fq_concat_i8_nhwc for one or two sources,
// fq_concat_n_i8_nhwc for up to eight).  What nested Concat markers compute, without the intermediate tensors: three nested
// two-source launches over branch widths a, b, c, d move 2(a+b) + 2(a+b+c) + 2(a+b+c+d) bytes per pixel, one launch 2(a+b+c+d).
//
//   base_i = C_0 + ... + C_{i-1}
//   out[n][h][w][c] = f_i(src_i[n][h / up_i][w / up_i][c - base_i])     base_i <= c < base_i + C_i
//                   = 0                                                  sum C <= c < Cpad_out
//   f_i = max(., 0) where relu_i == 1, the identity where relu_i == 0
//
// All operands stand for integer * 2^-g on the SAME grid g (the calibrator's merge group gives a Concat's operands one bit),
// so moving the integers is concatenating the values; nearest upsampling and ReLU commute with the scale.  No arithmetic
// worth the name: HBM bandwidth is the only resource: no LDS, no inline assembly, vector stores only.
// One kernel template, concat_i8_kernel<MAXSRC, GENERAL, UPS>, instantiated at MAXSRC = 2 and 8: the two-source launch keeps a
// parameter block of two entries and 8 waves per SIMD in every family, which the eight-entry general family does not reach.
//   * one lane owns one 16-byte chunk of the output (fq_concat_i8_geom.h) and stores it with one dwordx4; lanes run channel
//     fastest, so a wave stores whole contiguous pixels; at most 2048 workgroups of 256, a lane keeps its chunk index k and
//     strides over the pixels, so which sources it reads, at which offsets, under which masks is computed once per lane in front
//     of the pixel loop;
//   * GENERAL == false: every base_i % 16 == 0 (what models hit: branch widths in multiples of 16; every single-source call).
//     Every chunk is 16 bytes of one source at a 16-byte-aligned offset: one dwordx4 load, the tail mask, the ReLU, the store.
//     The owner's pointer, Cpad, offset, factor and ReLU mask are picked with a chain of selects over compile-time source indices
//     -- indexing the kernel arguments with a per-lane index would turn them into vector loads of the argument block;
//   * GENERAL == true: a chunk with one owner at a 16-byte-aligned source offset still takes that path; every other chunk is
//     or-ed together from the parts of every source with a byte in it.  A part is built from aligned dword loads and
//     v_alignbyte_b32 (a runtime byte shift of a 64-bit pair), masked to its own byte range and passed through its own ReLU
//     BEFORE the or: a source's padding bytes never reach the output.  A dword that holds no wanted byte is not loaded
//     (CatPart::ld), which is also what keeps the fifth dword of a row's last chunk inside the row.  The loop over the sources is
//     unrolled under the uniform guard i < nsrc, so every per-source value sits in registers (no scratch);
//   * UPS == true when a source is upsampled: the pixel is split into (n, h, w) once and source i reads (n, h >> lu_i, w >> lu_i);
//     neighbouring output pixels re-read the same source pixel from L1 / L2.  Without it source pixel == output pixel and the
//     loop holds no division.
// Every load is aligned and lies inside [q_i, q_i + N (H / up_i) (W / up_i) Cpad_i); scripts/concat_geom_check.cpp walks the
// same functions on the host over the tests' shapes, at both source limits.
#include "fq_common.h"
#include "fq_concat_i8_geom.h"

namespace fq {

template <int MAXSRC>
struct CatParams {
    CatGeom<MAXSRC> g;
    const int8_t* q[MAXSRC];
    unsigned relu_sign[MAXSRC];        // 0x80808080 where the source passes through a ReLU, else 0
};

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// max(byte, 0) on four int8 at once where sign = 0x80808080; the identity where sign = 0
__device__ __forceinline__ unsigned relu4(unsigned x, unsigned sign) { return x & ~(((x & sign) >> 7) * 0xffu); }

// The chunk k is 16 bytes of ONE source at a 16-byte-aligned offset of its pixel row.
template <int MAXSRC, bool UPS>
__device__ __forceinline__ void cat_loop16(int8_t* __restrict__ out, const CatParams<MAXSRC>& p, int k, unsigned pix, unsigned stride) {
    const CatGeom<MAXSRC>& g = p.g;
    const int8_t* __restrict__ src = p.q[0];
    int s = 0, hi = 16, lu = 0;
    unsigned cpad = 16u, sign = 0u;
#pragma unroll
    for (int i = 0; i < MAXSRC; ++i) {
        const CatPart pi = cat_part(g, k, i);
        const bool own = pi.use != 0;
        src = own ? p.q[i] : src;
        s = own ? pi.s : s;
        hi = own ? pi.hi : hi;
        lu = own ? g.s[i].lu : lu;
        cpad = own ? (unsigned)g.s[i].Cpad : cpad;
        sign = own ? p.relu_sign[i] : sign;
    }
    unsigned m[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) m[t] = cat_dword_mask(0, hi, t);
    for (; pix < g.npix; pix += stride) {
        unsigned sp = pix;
        if constexpr (UPS) {
            const unsigned w = pix % (unsigned)g.W, r = pix / (unsigned)g.W;
            sp = cat_src_pix(g, lu, r / (unsigned)g.H, r % (unsigned)g.H, w);
        }
        const v4u d = *reinterpret_cast<const v4u*>(src + (size_t)sp * cpad + s);
        v4u v;
        v.x = relu4(d.x & m[0], sign);
        v.y = relu4(d.y & m[1], sign);
        v.z = relu4(d.z & m[2], sign);
        v.w = relu4(d.w & m[3], sign);
        *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = v;
    }
}

template <int MAXSRC, bool GENERAL, bool UPS>
__global__ __launch_bounds__(kCatBlock) void concat_i8_kernel(int8_t* __restrict__ out, const CatParams<MAXSRC> p) {
    const CatGeom<MAXSRC>& g = p.g;
    const unsigned gid = blockIdx.x * kCatBlock + threadIdx.x;
    const unsigned stride = (gridDim.x * kCatBlock) / (unsigned)g.CH;
    const int k = (int)(gid % (unsigned)g.CH);
    unsigned pix = gid / (unsigned)g.CH;
    if (pix >= stride) return;

    if constexpr (!GENERAL) {
        cat_loop16<MAXSRC, UPS>(out, p, k, pix, stride);
    } else {
        int a[MAXSRC], sh[MAXSRC];
        unsigned ld[MAXSRC], m[MAXSRC][4];
        int owners = 0, whole = 0;
#pragma unroll
        for (int i = 0; i < MAXSRC; ++i) {
            const CatPart pi = cat_part(g, k, i);
            owners += pi.use;
            whole |= pi.use & pi.whole16;
            a[i] = pi.a;
            sh[i] = pi.sh;
            ld[i] = pi.ld;                                  // 0 where the source has no byte in the chunk
#pragma unroll
            for (int t = 0; t < 4; ++t) m[i][t] = pi.use ? cat_dword_mask(pi.lo, pi.hi, t) : 0u;
        }
        if (owners == 1 && whole) {
            cat_loop16<MAXSRC, UPS>(out, p, k, pix, stride);
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
                        const int8_t* row = p.q[i] + (size_t)sp * (unsigned)g.s[i].Cpad;
                        unsigned d[5];
#pragma unroll
                        for (int t = 0; t < 5; ++t) {
                            d[t] = 0u;
                            if (ld[i] & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (a[i] + 4 * t));
                        }
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            v[t] |= relu4(__builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)sh[i]) & m[i][t], p.relu_sign[i]);
                    }
                }
            }
            v4u o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = o;
        }
    }
}

static int log2_up(int up) { return up == 1 ? 0 : (up == 2 ? 1 : (up == 4 ? 2 : -1)); }

static bool cat_supported(const int* C, const int* up, int nsrc, int maxsrc) {
    if (!C || !up || nsrc < 1 || nsrc > maxsrc) return false;
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (C[i] < 1 || C[i] > 65536 || log2_up(up[i]) < 0) return false;
        sum += C[i];
    }
    return sum <= 65536;                                   // the chunks of one pixel fit the smallest launch
}

// the ReLU flag of one source: the two-source entry point has one flag for the whole call, the N-source one a field per source
static int src_relu(const fq_cat_src&, int relu) { return relu ? 1 : 0; }
static int src_relu(const fq_cat_src_n& s, int) { return s.relu; }

// Validation and launch of both entry points (SRC = fq_cat_src with the call's `relu`, or fq_cat_src_n).
template <int MAXSRC, class SRC>
static int cat_run(const SRC* srcs, int nsrc, int8_t* out, int Cpad_out, int relu, int N, int H, int W, fq_stream_t stream) {
    if (!srcs || nsrc < 1 || N < 0 || H <= 0 || W <= 0) return FQ_ERR_INVALID_ARG;
    if (nsrc > MAXSRC) return FQ_ERR_UNSUPPORTED;
    int C[MAXSRC], up[MAXSRC], rl[MAXSRC];
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        C[i] = srcs[i].C; up[i] = srcs[i].up; rl[i] = src_relu(srcs[i], relu);
        if (C[i] < 1 || up[i] < 1 || srcs[i].Cpad < C[i] || (rl[i] != 0 && rl[i] != 1)) return FQ_ERR_INVALID_ARG;
        sum += C[i];
    }
    if (!cat_supported(C, up, nsrc, MAXSRC)) return FQ_ERR_UNSUPPORTED;
    for (int i = 0; i < nsrc; ++i)
        if (srcs[i].Cpad % 16 || H % up[i] || W % up[i]) return FQ_ERR_UNSUPPORTED;
    if (Cpad_out != (int)((sum + 15) / 16 * 16)) return FQ_ERR_INVALID_ARG;
    if (nsrc == 1 && up[0] == 1 && !rl[0]) return FQ_ERR_INVALID_ARG;          // nothing to do
    if (N == 0) return FQ_OK;
    if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return FQ_ERR_INVALID_ARG;
    for (int i = 0; i < nsrc; ++i)
        if (!srcs[i].q || (reinterpret_cast<uintptr_t>(srcs[i].q) & 15u)) return FQ_ERR_INVALID_ARG;
    // 32-bit pixel and element arithmetic in the kernel
    if ((long)N * H * W * Cpad_out >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    for (int i = 0; i < nsrc; ++i)
        if ((long)N * (H / up[i]) * (W / up[i]) * srcs[i].Cpad >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    CatParams<MAXSRC> p;
    CatGeom<MAXSRC>& g = p.g;
    g.nsrc = nsrc;
    bool ups = false;
    int base = 0;
    for (int i = 0; i < MAXSRC; ++i) {
        const bool have = i < nsrc;
        g.s[i].C = have ? C[i] : 0;
        g.s[i].Cpad = have ? srcs[i].Cpad : 16;
        g.s[i].lu = have ? log2_up(up[i]) : 0;
        g.s[i].base = base;
        base += g.s[i].C;
        p.q[i] = have ? srcs[i].q : srcs[0].q;
        p.relu_sign[i] = have && rl[i] ? 0x80808080u : 0u;
        ups = ups || g.s[i].lu > 0;
    }
    g.N = N; g.H = H; g.W = W; g.Cpad_out = Cpad_out; g.CH = Cpad_out / 16;
    g.npix = (unsigned)((long)N * H * W);
    const bool general = !cat_aligned(g);
    const unsigned blocks = (unsigned)cat_blocks(g);
    hipStream_t st = as_stream(stream);
    if (general) {
        if (ups) concat_i8_kernel<MAXSRC, true, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_i8_kernel<MAXSRC, true, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    } else {
        if (ups) concat_i8_kernel<MAXSRC, false, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_i8_kernel<MAXSRC, false, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_concat_i8_nhwc_supported(const int* C, const int* up, int nsrc) { return cat_supported(C, up, nsrc, 2) ? 1 : 0; }
extern "C" int fq_concat_n_i8_nhwc_supported(const int* C, const int* up, int nsrc) {
    return cat_supported(C, up, nsrc, FQ_CONCAT_N_MAX_SRC) ? 1 : 0;
}

extern "C" int fq_concat_i8_nhwc(const fq_cat_src* srcs, int nsrc, int8_t* out, int Cpad_out, int relu, int N, int H, int W,
                                 fq_stream_t stream) {
    return cat_run<2>(srcs, nsrc, out, Cpad_out, relu, N, H, W, stream);
}

extern "C" int fq_concat_n_i8_nhwc(const fq_cat_src_n* srcs, int nsrc, int8_t* out, int Cpad_out, int N, int H, int W,
                                   fq_stream_t stream) {
    return cat_run<FQ_CONCAT_N_MAX_SRC>(srcs, nsrc, out, Cpad_out, 0, N, H, W, stream);
}
