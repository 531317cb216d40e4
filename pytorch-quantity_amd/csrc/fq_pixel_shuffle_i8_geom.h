// fq_pixel_shuffle_i8_geom.h -- the host guards, the launch geometry and the index arithmetic of the int8 NHWC pixel shuffle /
// unshuffle (fq_pixel_shuffle_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/pixel_shuffle_geom_check.cpp walks them, lane by lane, over the shapes the GPU tests and the model launch.
//
//   inverse == 0 (nn.PixelShuffle(r)):    y[n][h r + i][w r + j][c] = x[n][h][w][c r^2 + i r + j]      0 <= c < C
//   inverse == 1 (nn.PixelUnshuffle(r)):  y[n][h][w][c r^2 + i r + j] = x[n][h r + i][w r + j][c]
//   padding channels of y are zero.  H, W: the LOW-resolution plane in both directions.
//
// Two tensors, two views.  The DEEP one has r^2 C real channels on the low-resolution plane (the source of a shuffle, the output
// of an unshuffle), the SHALLOW one C real channels on the r times larger plane.
//
// Aligned family (r in {2, 4}, C % 16 == 0: no padding anywhere).  An ITEM is (low-resolution pixel, k): the 16 channels
//   [16 k, 16 k + 16) of the shallow tensor at the r^2 positions of that pixel, which are the 16 r^2 CONSECUTIVE bytes
//   [16 r^2 k, 16 r^2 (k + 1)) of the deep pixel.  One lane loads r^2 dwordx4, transposes bytes in registers (ps_transpose4: eight
//   v_perm_b32 per 4 x 4 bytes) and stores r^2 dwordx4.  ps_deep_off / ps_shallow_off name the two sides' byte offsets.
// General family (r == 3, or C % 16 != 0).  An ITEM is one 16-byte chunk of the OUTPUT in memory order (store offset 16 * item:
//   a wave stores 1 KiB contiguously).  Each of its bytes below the real width comes from one aligned dword load of the source
//   (ps_gen_src names the byte); the rest are zero without a read.
// Both: at most kPsMaxBlocks workgroups of kPsBlock lanes; a lane takes items lane, lane + stride, ...  The item is split into
// (row, w, k) by division ONCE (ps_walk_begin); ps_walk_step then advances the three digits by the stride's own digits with two
// carries.  Divisions by r or r^2 are divisions by a template constant in the kernel.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FQ_PS_HD __host__ __device__ __forceinline__
#define FQ_PS_UNROLL _Pragma("unroll")
#else
#define FQ_PS_HD inline
#define FQ_PS_UNROLL
#endif

namespace fq {

constexpr int kPsBlock = 256;             // threads per workgroup
constexpr int kPsMaxBlocks = 2048;        // 256 CUs x 8 workgroups: lanes stride over the rest of the items
constexpr int kPsMaxDeepC = 65536;        // C r^2 above this is not taken
constexpr int kPsOk = 0, kPsInvalid = -1, kPsUnsupported = -4;      // FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED (include/fq.h)
constexpr int kPsAligned = 1, kPsGeneral = 2;

FQ_PS_HD int ps_pad16(int c) { return (c + 15) / 16 * 16; }

// 0: not taken; kPsAligned / kPsGeneral: the family that runs (C, r).  `inverse` does not change the family.
FQ_PS_HD int ps_family(int C, int r, int inverse) {
    if (C < 1 || r < 2 || r > 4 || inverse < 0 || inverse > 1 || (long)C * r * r > kPsMaxDeepC) return 0;
    return (r != 3 && C % 16 == 0) ? kPsAligned : kPsGeneral;
}

// The entry point's verdict on everything but the launch itself: scalars first, then N == 0, then the pointers (given as
// addresses).  kPsOk with *launch == 0: nothing to do (N == 0).
FQ_PS_HD int ps_guard(uintptr_t x, int Cpad_in, uintptr_t y, int Cpad_out, int C, int r, int inverse, int N, int H, int W,
                      int* launch) {
    *launch = 0;
    if (N < 0 || H < 1 || W < 1 || C < 1 || inverse < 0 || inverse > 1) return kPsInvalid;
    if (r < 2 || r > 4) return kPsUnsupported;
    if ((long)C * r * r > kPsMaxDeepC) return kPsUnsupported;
    const int deep = ps_pad16(C * r * r), shallow = ps_pad16(C);
    if (Cpad_in != (inverse ? shallow : deep) || Cpad_out != (inverse ? deep : shallow)) return kPsInvalid;
    // 32-bit byte offsets in the kernel: both tensors below 2^31 - 1 bytes
    long npix = (long)N * H;
    if (npix >= 0x7fffffffL) return kPsUnsupported;
    npix *= W;
    if (npix >= 0x7fffffffL || npix * deep >= 0x7fffffffL || npix * r * r >= 0x7fffffffL || npix * r * r * shallow >= 0x7fffffffL)
        return kPsUnsupported;
    if (N == 0) return kPsOk;
    if (!x || !y || (x & 15u) || (y & 15u)) return kPsInvalid;
    *launch = 1;
    return kPsOk;
}

struct PsGeom {
    int C, r, inverse, family;
    int Cdeep, Cshal;                      // row bytes of the deep / shallow tensor: pad16(C r^2), pad16(C)
    unsigned H, W;                         // the low-resolution plane
    unsigned CH;                           // chunks per walked pixel: aligned C / 16, general Cpad_out / 16
    unsigned Wd;                           // pixels per walked row: W, or (general shuffle: the output is the shallow tensor) W r
    unsigned items, blocks, stride;        // stride = blocks * kPsBlock
    unsigned dk, dw, drow;                 // stride = (drow * Wd + dw) * CH + dk
};

// (a geometry the guard took, N >= 1)
FQ_PS_HD PsGeom ps_geom(int C, int r, int inverse, int N, int H, int W) {
    PsGeom g;
    g.C = C; g.r = r; g.inverse = inverse; g.family = ps_family(C, r, inverse);
    g.Cdeep = ps_pad16(C * r * r); g.Cshal = ps_pad16(C);
    g.H = (unsigned)H; g.W = (unsigned)W;
    unsigned rows = (unsigned)N * (unsigned)H;
    if (g.family == kPsAligned) {
        g.CH = (unsigned)C / 16u; g.Wd = g.W;
    } else if (inverse) {
        g.CH = (unsigned)g.Cdeep / 16u; g.Wd = g.W;
    } else {
        g.CH = (unsigned)g.Cshal / 16u; g.Wd = g.W * (unsigned)r; rows *= (unsigned)r;
    }
    g.items = rows * g.Wd * g.CH;
    const unsigned want = (g.items + (unsigned)kPsBlock - 1u) / (unsigned)kPsBlock;
    g.blocks = want > (unsigned)kPsMaxBlocks ? (unsigned)kPsMaxBlocks : want;
    g.stride = g.blocks * (unsigned)kPsBlock;
    g.dk = g.stride % g.CH;
    const unsigned pix = g.stride / g.CH;
    g.dw = pix % g.Wd; g.drow = pix / g.Wd;
    return g;
}

// item = (row * Wd + w) * CH + k
struct PsWalk {
    unsigned row, w, k;
};
FQ_PS_HD PsWalk ps_walk_begin(const PsGeom& g, unsigned item) {
    PsWalk s;
    const unsigned pix = item / g.CH;
    s.k = item - pix * g.CH;
    s.row = pix / g.Wd;
    s.w = pix - s.row * g.Wd;
    return s;
}
FQ_PS_HD void ps_walk_step(const PsGeom& g, PsWalk& s) {
    s.k += g.dk;
    if (s.k >= g.CH) { s.k -= g.CH; ++s.w; }
    s.w += g.dw;
    if (s.w >= g.Wd) { s.w -= g.Wd; ++s.row; }
    s.row += g.drow;
}

// ---- aligned family: the two sides of item (row, w, k), position q = i r + j
// deep tensor: the q-th 16 bytes of the item's 16 r^2 consecutive ones
FQ_PS_HD size_t ps_deep_off(const PsGeom& g, unsigned item, int q, int R) { return ((size_t)item * (size_t)(R * R) + (size_t)q) * 16u; }
// shallow tensor: chunk k of pixel (row r + i, w r + j)
FQ_PS_HD size_t ps_shallow_off(const PsGeom& g, const PsWalk& s, int i, int j, int R) {
    const size_t pixel = ((size_t)s.row * (size_t)R + (size_t)i) * ((size_t)g.W * (size_t)R) + (size_t)s.w * (size_t)R + (size_t)j;
    return pixel * (size_t)g.Cshal + 16u * (size_t)s.k;
}

// v_perm_b32: byte n of the result is byte sel[n] of the eight bytes {hi, lo} (0 .. 3: lo, 4 .. 7: hi)
FQ_PS_HD unsigned ps_perm(unsigned hi, unsigned lo, unsigned sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const unsigned long long both = ((unsigned long long)hi << 32) | lo;
    unsigned out = 0;
    for (int n = 0; n < 4; ++n) out |= (unsigned)((both >> (8 * ((sel >> (8 * n)) & 7u))) & 0xffu) << (8 * n);
    return out;
#endif
}

// t[q] byte m = a[m] byte q: a 4 x 4 byte transpose
FQ_PS_HD void ps_transpose4(unsigned a0, unsigned a1, unsigned a2, unsigned a3, unsigned (&t)[4]) {
    const unsigned lo01 = ps_perm(a1, a0, 0x05010400u), hi01 = ps_perm(a1, a0, 0x07030602u);
    const unsigned lo23 = ps_perm(a3, a2, 0x05010400u), hi23 = ps_perm(a3, a2, 0x07030602u);
    t[0] = ps_perm(lo23, lo01, 0x05040100u);
    t[1] = ps_perm(lo23, lo01, 0x07060302u);
    t[2] = ps_perm(hi23, hi01, 0x05040100u);
    t[3] = ps_perm(hi23, hi01, 0x07060302u);
}

struct PsV4 {
    unsigned d[4];
};

// deep -> shallow, r = 2.  in[m] dword e is channel 4 m + e of the chunk with its four positions as bytes; out[q] is position q.
FQ_PS_HD void ps_net2_d2s(const PsV4 (&in)[4], PsV4 (&out)[4]) {
    FQ_PS_UNROLL
    for (int m = 0; m < 4; ++m) {
        unsigned t[4];
        ps_transpose4(in[m].d[0], in[m].d[1], in[m].d[2], in[m].d[3], t);
        FQ_PS_UNROLL
        for (int q = 0; q < 4; ++q) out[q].d[m] = t[q];
    }
}
// shallow -> deep, r = 2.  in[q] is position q; out[m] dword e is channel 4 m + e.
FQ_PS_HD void ps_net2_s2d(const PsV4 (&in)[4], PsV4 (&out)[4]) {
    FQ_PS_UNROLL
    for (int m = 0; m < 4; ++m) {
        unsigned t[4];
        ps_transpose4(in[0].d[m], in[1].d[m], in[2].d[m], in[3].d[m], t);
        FQ_PS_UNROLL
        for (int e = 0; e < 4; ++e) out[m].d[e] = t[e];
    }
}
// r = 4, both directions (the network is its own inverse): one side has one dwordx4 per channel with the 16 positions as bytes,
// the other one dwordx4 per position with the 16 channels as bytes.  out[4 Y + t] dword X byte e = in[4 X + e] dword Y byte t.
FQ_PS_HD void ps_net4(const PsV4 (&in)[16], PsV4 (&out)[16]) {
    FQ_PS_UNROLL
    for (int Y = 0; Y < 4; ++Y)
        FQ_PS_UNROLL
        for (int X = 0; X < 4; ++X) {
            unsigned t[4];
            ps_transpose4(in[4 * X].d[Y], in[4 * X + 1].d[Y], in[4 * X + 2].d[Y], in[4 * X + 3].d[Y], t);
            FQ_PS_UNROLL
            for (int e = 0; e < 4; ++e) out[4 * Y + e].d[X] = t[e];
        }
}

// ---- general family: output chunk k of walked pixel (row, w); its byte b is output channel 16 k + b
// is that byte a real channel?  (the others are zero without a read)
FQ_PS_HD bool ps_gen_real(const PsGeom& g, const PsWalk& s, int b) {
    return 16u * s.k + (unsigned)b < (unsigned)(g.inverse ? g.C * g.r * g.r : g.C);
}
// the byte offset in x of a real byte.  R == g.r (a constant in the kernel: every division below is by a constant)
FQ_PS_HD size_t ps_gen_src(const PsGeom& g, const PsWalk& s, int b, int R) {
    const unsigned c = 16u * s.k + (unsigned)b;
    if (!g.inverse) {
        // (row, w) is a pixel of the shallow output: row = (n H + h) R + i, w = wl R + j
        const unsigned lo_row = s.row / (unsigned)R, i = s.row - lo_row * (unsigned)R;
        const unsigned wl = s.w / (unsigned)R, j = s.w - wl * (unsigned)R;
        return ((size_t)lo_row * (size_t)g.W + (size_t)wl) * (size_t)g.Cdeep + (size_t)c * (size_t)(R * R) + (size_t)(i * (unsigned)R + j);
    }
    // (row, w) is a pixel of the deep output: channel c = cs R^2 + i R + j reads the shallow pixel (row R + i, w R + j)
    const unsigned cs = c / (unsigned)(R * R), q = c - cs * (unsigned)(R * R);
    const unsigned i = q / (unsigned)R, j = q - i * (unsigned)R;
    const size_t pixel = ((size_t)s.row * (size_t)R + (size_t)i) * ((size_t)g.W * (size_t)R) + (size_t)s.w * (size_t)R + (size_t)j;
    return pixel * (size_t)g.Cshal + (size_t)cs;
}

}  // namespace fq
