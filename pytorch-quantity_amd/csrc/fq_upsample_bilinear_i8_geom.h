// fq_upsample_bilinear_i8_geom.h -- the lane -> (source item, taps, weights, output offsets) arithmetic of the resident int8
// bilinear upsampling (fq_upsample_bilinear_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/upsample_bilinear_geom_check.cpp walks them over the shapes the GPU tests and the U-Net model run and asserts that every
// load lies inside the source and is 16-byte aligned, that every output element is written exactly once, and that taps and weights
// are the closed form of include/fq.h.
//
// x is [N][H][W][Cpad], y is [N][up H][up W][Cpad]; up is 2 or 4, D = 2 up.  An ITEM is 16 consecutive channels of one SOURCE
// pixel, CH = Cpad / 16 items per pixel, item i = ((n H + h) W + w) CH + k: channel fastest, then w.  The lane that owns an item
// writes the up x up output pixels (up h + dy, up w + dx) at those channels.  With align_corners=False output row o = up h + dy
// reads
//   t = max(2 o + 1 - up, 0),  i0 = t div D,  l1 = t mod D,  l0 = D - l1,  i1 = min(i0 + 1, H - 1)
// and, written per (h, dy) with a = 2 dy + 1 - up (odd, |a| < up):
//   a < 0:  rows (max(h - 1, 0), h)      weights (-a, D + a)      -- at h = 0 both taps are row 0 and the weights add up to D,
//   a > 0:  rows (h, min(h + 1, H - 1))  weights (D - a, a)          which is what the clamp of t to 0 gives
// so the taps of all up x up outputs lie in the 3 x 3 neighbourhood of (h, w) with its indices clamped to the plane (upb_nbr), and
// the weights depend on (dy, dx) alone (upb_tap): compile-time constants in the kernel.  Columns follow the same rule.
//
// The lane -> item map is fq_add_up_geom.h's: lane t (global index) takes the items t, t + S, t + 2 S, ... with S the launch's
// lane count; only the first item of a lane is split by division (upb_first), every further one by adding the split of S digit
// by digit (upb_next).  Byte offsets are 32-bit: the entry point refuses an output of 2^31 - 1 bytes or more.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define FQ_UPB_HD __host__ __device__ __forceinline__
#else
#define FQ_UPB_HD inline
#endif

namespace fq {

constexpr int kUpbBlock = 256;                   // threads per workgroup
constexpr int kUpbMaxBlocks = 256 * 16;          // 16 workgroups for each of the 256 CUs
constexpr int kUpbMaxShift = 8;                  // |b - g|
constexpr long kUpbMaxBytes = 0x7ffffffeL;       // the output: 32-bit byte offsets, as the other int8 NHWC entry points

struct UpbItem { int n, h, w, k; };

struct UpbGeom {
    int N, H, W, C, Cpad, CH;          // source plane, CH = Cpad / 16
    int up, Ho, Wo;                    // factor, output plane
    unsigned items;                    // N H W CH
    UpbItem step;                      // the launch's stride S split as (S / (H W CH), S / (W CH) % H, S / CH % W, S % CH)
};

struct UpbNbr { int row[3], col[3]; };           // (h - 1, h, h + 1) and (w - 1, w, w + 1), clamped to the plane

struct UpbTap { int first, l0, l1; };            // taps nbr[first] and nbr[first + 1] with weights l0 and l1, l0 + l1 = D

struct UpbRound { int rsh, lsh, bias, lo; };     // r = S * 2^e: e < 0 -> rsh = -e, bias = 2^(rsh - 1) - 1; e >= 0 -> lsh = e

FQ_UPB_HD int upb_log2(int up) { return up == 2 ? 1 : (up == 4 ? 2 : -1); }

FQ_UPB_HD bool upb_supported(int up, int shift) { return upb_log2(up) > 0 && shift >= -kUpbMaxShift && shift <= kUpbMaxShift; }

// status of the scalar arguments: 0 fine, -1 invalid, -4 not taken (FQ_ERR_INVALID_ARG / FQ_ERR_UNSUPPORTED); N == 0 is fine
FQ_UPB_HD int upb_args(int N, int H, int W, int C, int Cpad, int up, int shift) {
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || Cpad <= 0 || C > Cpad || (Cpad & 15)) return -1;
    if (!upb_supported(up, shift)) return -4;
    long n = (long)N * up * up;                              // each factor is below 2^31 and the product is checked after each
    if (n > kUpbMaxBytes) return -4;
    n *= H;
    if (n > kUpbMaxBytes) return -4;
    n *= W;
    if (n > kUpbMaxBytes) return -4;
    n *= Cpad;
    return n > kUpbMaxBytes ? -4 : 0;
}

// e = shift - 2 log2(D): the one rounding of the rule (include/fq.h), as shift amounts
FQ_UPB_HD UpbRound upb_round(int up, int shift, int relu) {
    const int e = shift - 2 * (upb_log2(up) + 1);
    UpbRound r;
    r.rsh = e < 0 ? -e : 0;
    r.lsh = e > 0 ? e : 0;
    r.bias = r.rsh > 0 ? (1 << (r.rsh - 1)) - 1 : 0;
    r.lo = relu ? 0 : -128;
    return r;
}

// The rule on one sum, in plain integers (the kernel does the same on packed int16; |S| <= 128 D^2 <= 8192, rsh <= 14, so
// S + bias + 1 <= 16384 stays inside int16).  Half to even: add 2^(rsh-1) - 1 and the bit that will become the lowest.
FQ_UPB_HD int upb_requant(int S, const UpbRound& r) {
    int v;
    if (r.rsh > 0) {
        v = (S + r.bias + ((S >> r.rsh) & 1)) >> r.rsh;
    } else {
        v = S < -128 ? -128 : (S > 127 ? 127 : S);           // (clamping first keeps the left shift inside int16; it is monotone)
        v = v * (1 << r.lsh);
    }
    return v < r.lo ? r.lo : (v > 127 ? 127 : v);
}

// workgroups of one launch: one lane per item up to the cap, at least one
FQ_UPB_HD unsigned upb_blocks(unsigned items) {
    unsigned b = (items + (unsigned)kUpbBlock - 1u) / (unsigned)kUpbBlock;
    if (b > (unsigned)kUpbMaxBlocks) b = (unsigned)kUpbMaxBlocks;
    return b ? b : 1u;
}

// item i split into its digits (division: once per lane, and once per launch for the stride)
FQ_UPB_HD UpbItem upb_split(int H, int W, int CH, unsigned i) {
    UpbItem c;
    c.k = (int)(i % (unsigned)CH);
    unsigned r = i / (unsigned)CH;
    c.w = (int)(r % (unsigned)W);
    r /= (unsigned)W;
    c.h = (int)(r % (unsigned)H);
    c.n = (int)(r / (unsigned)H);
    return c;
}

FQ_UPB_HD UpbGeom upb_geom(int N, int H, int W, int C, int Cpad, int up) {
    UpbGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.Cpad = Cpad; g.CH = Cpad / 16;
    g.up = up; g.Ho = up * H; g.Wo = up * W;
    g.items = (unsigned)((long)N * H * W * g.CH);
    g.step = upb_split(H, W, g.CH, upb_blocks(g.items) * (unsigned)kUpbBlock);
    return g;
}

FQ_UPB_HD UpbItem upb_first(const UpbGeom& g, unsigned i) { return upb_split(g.H, g.W, g.CH, i); }

// the item S further on: digit-wise addition, every digit of both summands is below its base, so one carry at most
FQ_UPB_HD UpbItem upb_next(const UpbGeom& g, UpbItem c) {
    c.k += g.step.k;
    int carry = c.k >= g.CH;
    c.k -= carry ? g.CH : 0;
    c.w += g.step.w + carry;
    carry = c.w >= g.W;
    c.w -= carry ? g.W : 0;
    c.h += g.step.h + carry;
    carry = c.h >= g.H;
    c.h -= carry ? g.H : 0;
    c.n += g.step.n + carry;
    return c;
}

FQ_UPB_HD UpbNbr upb_nbr(const UpbGeom& g, const UpbItem& c) {
    UpbNbr nb;
    nb.row[0] = c.h > 0 ? c.h - 1 : 0;
    nb.row[1] = c.h;
    nb.row[2] = c.h + 1 < g.H ? c.h + 1 : g.H - 1;
    nb.col[0] = c.w > 0 ? c.w - 1 : 0;
    nb.col[1] = c.w;
    nb.col[2] = c.w + 1 < g.W ? c.w + 1 : g.W - 1;
    return nb;
}

// taps and weights of sub-position d (0 <= d < up) along one axis
FQ_UPB_HD constexpr UpbTap upb_tap(int up, int d) {
    const int a = 2 * d + 1 - up, D = 2 * up;
    return a < 0 ? UpbTap{0, -a, D + a} : UpbTap{1, D - a, a};
}

// byte offset of the 16 channels k of source pixel (n, row, col)
FQ_UPB_HD unsigned upb_src_offset(const UpbGeom& g, int n, int row, int col, int k) {
    return (((unsigned)n * (unsigned)g.H + (unsigned)row) * (unsigned)g.W + (unsigned)col) * (unsigned)g.Cpad + 16u * (unsigned)k;
}

// byte offset of the 16 channels k of output pixel (n, up h + dy, up w + dx)
FQ_UPB_HD unsigned upb_dst_offset(const UpbGeom& g, const UpbItem& c, int dy, int dx) {
    const unsigned oh = (unsigned)(g.up * c.h + dy), ow = (unsigned)(g.up * c.w + dx);
    return (((unsigned)c.n * (unsigned)g.Ho + oh) * (unsigned)g.Wo + ow) * (unsigned)g.Cpad + 16u * (unsigned)c.k;
}

// byte mask of dword t (0 .. 3) of the 16 channels k: 0xff where the channel is a real one (< C)
FQ_UPB_HD unsigned upb_dword_mask(const UpbGeom& g, int k, int t) {
    const int first = 16 * k + 4 * t;
    const int real = g.C - first;
    return real >= 4 ? 0xffffffffu : (real <= 0 ? 0u : (1u << (8 * real)) - 1u);
}

}  // namespace fq
