// fq_concat_i8.hip -- channel concatenation and nearest upsampling of resident int8 NHWC activations (include/fq.h:
// fq_concat_i8_nhwc).
//
//   out[n][h][w][c] = src0[n][h / up0][w / up0][c]          c <  C0
//                   = src1[n][h / up1][w / up1][c - C0]     C0 <= c < C0 + C1
//                   = 0                                     C0 + C1 <= c < Cpad_out          (then max(., 0) when relu != 0)
//
// Both operands stand for integer * 2^-g on the SAME grid g (the calibrator's merge group gives a Concat's operands one bit),
// so moving the integers is concatenating the values; nearest upsampling and ReLU commute with the scale.  No arithmetic
// worth the name: HBM bandwidth is the only resource, there is no LDS.
//   * one lane owns one 16-byte chunk of the output (fq_concat_i8_geom.h) and stores it with one dwordx4; lanes run channel
//     fastest, so a wave stores whole contiguous pixels; at most 2048 workgroups, a lane keeps its chunk index k and strides
//     over the pixels, so which source(s) it reads, at which byte offset, under which masks is computed once per lane;
//   * GENERAL == false is the case C0 % 16 == 0 (and every single-source call): every chunk is 16 bytes of one source at a
//     16-byte-aligned offset -- one dwordx4 load, the mask only cuts the channels behind the last source;
//   * GENERAL == true (C0 % 16 != 0): chunks wholly inside src0 are still one dwordx4 load; every other chunk is put together
//     from aligned dword loads of either source with v_alignbyte_b32 (a runtime byte shift of a 64-bit pair), masked at C0 and
//     at C0 + C1 BEFORE the two parts are or-ed: a source's padding bytes never reach the output.  A dword that holds no
//     wanted byte is not loaded (CatPart::ld), which is also what keeps the fifth dword of a row's last chunk inside the row;
//   * UPS == true when an operand is upsampled: the pixel is split into (n, h, w) and the source pixel is (n, h >> lu, w >> lu);
//     neighbouring output pixels re-read the same source pixel from L1 / L2.  Without it source pixel == output pixel and the
//     loop holds no division.
// Every load is aligned and lies inside [q_i, q_i + N (H / up_i) (W / up_i) Cpad_i); scripts/concat_geom_check.cpp walks the
// same functions on the host over the tests' shapes.
#include "fq_common.h"
#include "fq_concat_i8_geom.h"

namespace fq {

struct CatParams {
    CatGeom g;
    const int8_t* q[kCatMaxSrc];
    unsigned relu_sign;                // 0x80808080 with the fused ReLU, else 0
};

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// max(byte, 0) on four int8 at once where sign = 0x80808080; the identity where sign = 0
__device__ __forceinline__ unsigned relu4(unsigned x, unsigned sign) { return x & ~(((x & sign) >> 7) * 0xffu); }

template <bool GENERAL, bool UPS>
__global__ __launch_bounds__(kCatBlock) void concat_i8_kernel(int8_t* __restrict__ out, const CatParams p) {
    const CatGeom& g = p.g;
    const unsigned gid = blockIdx.x * kCatBlock + threadIdx.x;
    const unsigned stride = (gridDim.x * kCatBlock) / (unsigned)g.CH;
    const int k = (int)(gid % (unsigned)g.CH);
    unsigned pix = gid / (unsigned)g.CH;
    if (pix >= stride) return;

    if constexpr (!GENERAL) {
        // exactly one source owns the chunk, at a 16-byte-aligned offset of its pixel row (the fields are picked with selects,
        // not by indexing the kernel arguments with a per-lane index: those would become vector loads of the argument block)
        const CatPart p0 = cat_part(g, k, 0), p1 = cat_part(g, k, 1);
        const bool second = p1.use;
        const int s = second ? p1.s : p0.s, hi = second ? p1.hi : p0.hi, lu = second ? g.s[1].lu : g.s[0].lu;
        const int8_t* __restrict__ src = second ? p.q[1] : p.q[0];
        const unsigned cpad = (unsigned)(second ? g.s[1].Cpad : g.s[0].Cpad);
        unsigned m[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) m[t] = cat_dword_mask(0, hi, t);
        for (; pix < g.npix; pix += stride) {
            const unsigned sp = UPS ? cat_src_pix_lu(g, lu, pix) : pix;
            const v4u d = *reinterpret_cast<const v4u*>(src + (size_t)sp * cpad + s);
            v4u v;
            v.x = relu4(d.x & m[0], p.relu_sign);
            v.y = relu4(d.y & m[1], p.relu_sign);
            v.z = relu4(d.z & m[2], p.relu_sign);
            v.w = relu4(d.w & m[3], p.relu_sign);
            *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = v;
        }
    } else {
        const CatPart p0 = cat_part(g, k, 0), p1 = cat_part(g, k, 1);
        const int8_t* __restrict__ s0 = p.q[0];
        const int8_t* __restrict__ s1 = p.q[1];
        if (p0.whole16 && !p1.use) {
            // wholly inside src0 (C0 % 16 != 0 here: a chunk of src1 never starts on a 16-byte boundary)
            for (; pix < g.npix; pix += stride) {
                const unsigned sp = UPS ? cat_src_pix(g, 0, pix) : pix;
                const v4u d = *reinterpret_cast<const v4u*>(s0 + (size_t)sp * g.s[0].Cpad + p0.s);
                v4u v;
                v.x = relu4(d.x, p.relu_sign);
                v.y = relu4(d.y, p.relu_sign);
                v.z = relu4(d.z, p.relu_sign);
                v.w = relu4(d.w, p.relu_sign);
                *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = v;
            }
            return;
        }
        unsigned m0[4], m1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            m0[t] = p0.use ? cat_dword_mask(p0.lo, p0.hi, t) : 0u;
            m1[t] = p1.use ? cat_dword_mask(p1.lo, p1.hi, t) : 0u;
        }
        for (; pix < g.npix; pix += stride) {
            unsigned v[4] = {0u, 0u, 0u, 0u};
            if (p0.use) {
                const unsigned sp = UPS ? cat_src_pix(g, 0, pix) : pix;
                const int8_t* row = s0 + (size_t)sp * g.s[0].Cpad;
                unsigned d[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    d[t] = 0u;
                    if (p0.ld & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (p0.a + 4 * t));
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)p0.sh) & m0[t];
            }
            if (p1.use) {
                const unsigned sp = UPS ? cat_src_pix(g, 1, pix) : pix;
                const int8_t* row = s1 + (size_t)sp * g.s[1].Cpad;
                unsigned d[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    d[t] = 0u;
                    if (p1.ld & (1u << t)) d[t] = *reinterpret_cast<const unsigned*>(row + (p1.a + 4 * t));
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] |= __builtin_amdgcn_alignbyte(d[t + 1], d[t], (unsigned)p1.sh) & m1[t];
            }
            v4u o;
            o.x = relu4(v[0], p.relu_sign);
            o.y = relu4(v[1], p.relu_sign);
            o.z = relu4(v[2], p.relu_sign);
            o.w = relu4(v[3], p.relu_sign);
            *reinterpret_cast<v4u*>(out + (size_t)pix * g.Cpad_out + 16 * k) = o;
        }
    }
}

static int log2_up(int up) { return up == 1 ? 0 : (up == 2 ? 1 : (up == 4 ? 2 : -1)); }

static bool cat_supported(const int* C, const int* up, int nsrc) {
    if (!C || !up || nsrc < 1 || nsrc > kCatMaxSrc) return false;
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (C[i] < 1 || C[i] > 65536 || log2_up(up[i]) < 0) return false;
        sum += C[i];
    }
    return sum <= 65536;                                   // the chunks of one pixel fit the smallest launch
}

}  // namespace fq

using namespace fq;

extern "C" int fq_concat_i8_nhwc_supported(const int* C, const int* up, int nsrc) { return cat_supported(C, up, nsrc) ? 1 : 0; }

extern "C" int fq_concat_i8_nhwc(const fq_cat_src* srcs, int nsrc, int8_t* out, int Cpad_out, int relu, int N, int H, int W,
                                 fq_stream_t stream) {
    if (!srcs || nsrc < 1 || N < 0 || H <= 0 || W <= 0) return FQ_ERR_INVALID_ARG;
    if (nsrc > kCatMaxSrc) return FQ_ERR_UNSUPPORTED;
    int C[kCatMaxSrc], up[kCatMaxSrc];
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        C[i] = srcs[i].C; up[i] = srcs[i].up;
        if (C[i] < 1 || up[i] < 1 || srcs[i].Cpad < C[i]) return FQ_ERR_INVALID_ARG;
        sum += C[i];
    }
    if (!cat_supported(C, up, nsrc)) return FQ_ERR_UNSUPPORTED;
    for (int i = 0; i < nsrc; ++i)
        if (srcs[i].Cpad % 16 || H % up[i] || W % up[i]) return FQ_ERR_UNSUPPORTED;
    if (Cpad_out != (int)((sum + 15) / 16 * 16)) return FQ_ERR_INVALID_ARG;
    if (nsrc == 1 && up[0] == 1 && !relu) return FQ_ERR_INVALID_ARG;          // nothing to do
    if (N == 0) return FQ_OK;
    if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return FQ_ERR_INVALID_ARG;
    for (int i = 0; i < nsrc; ++i)
        if (!srcs[i].q || (reinterpret_cast<uintptr_t>(srcs[i].q) & 15u)) return FQ_ERR_INVALID_ARG;
    // 32-bit pixel and element arithmetic in the kernel
    if ((long)N * H * W * Cpad_out >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    for (int i = 0; i < nsrc; ++i)
        if ((long)N * (H / up[i]) * (W / up[i]) * srcs[i].Cpad >= 0x7fffffffL) return FQ_ERR_UNSUPPORTED;
    CatParams p;
    CatGeom& g = p.g;
    g.nsrc = nsrc;
    bool ups = false;
    for (int i = 0; i < kCatMaxSrc; ++i) {
        const bool have = i < nsrc;
        g.s[i].C = have ? C[i] : 0;
        g.s[i].Cpad = have ? srcs[i].Cpad : 16;
        g.s[i].lu = have ? log2_up(up[i]) : 0;
        p.q[i] = have ? srcs[i].q : srcs[0].q;
        ups = ups || g.s[i].lu > 0;
    }
    g.N = N; g.H = H; g.W = W; g.Cpad_out = Cpad_out; g.CH = Cpad_out / 16;
    g.npix = (unsigned)((long)N * H * W);
    p.relu_sign = relu ? 0x80808080u : 0u;
    const bool general = nsrc == 2 && (C[0] % 16) != 0;
    const unsigned blocks = (unsigned)cat_blocks(g);
    hipStream_t st = as_stream(stream);
    if (general) {
        if (ups) concat_i8_kernel<true, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_i8_kernel<true, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    } else {
        if (ups) concat_i8_kernel<false, true><<<blocks, kCatBlock, 0, st>>>(out, p);
        else concat_i8_kernel<false, false><<<blocks, kCatBlock, 0, st>>>(out, p);
    }
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
