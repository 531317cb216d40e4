// fq_concat_i8_geom.h -- the lane -> (sources, offsets, masks, loads) arithmetic of the int8 NHWC concatenation / nearest
// upsampling (fq_concat_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/concat_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every load lies inside its source
// and every output chunk is written exactly once.
//
// The output is [N][H][W][Cpad_out] bytes; a CHUNK is 16 consecutive channels of one pixel (one dwordx4 store), CH = Cpad_out / 16
// chunks per pixel.  Chunk k holds output channels [16k, 16k + 16).  Source i owns output channels [base_i, base_i + C_i),
// base_i = C_0 + ... + C_{i-1}; relative to the source's pixel row the chunk starts at byte s = 16k - base_i (negative when the
// chunk begins in a source before), so one chunk may hold bytes of every source.  A lane keeps k for its whole life, so
// everything below except the pixel is per-lane constant.
//
// Everything is a template on MAXSRC, the number of source entries of the kernel's parameter block: the kernel is instantiated
// at 2 (fq_concat_i8_nhwc) and at 8 (fq_concat_n_i8_nhwc), and the two-source launch carries two entries, not eight.
#pragma once

#if defined(__HIPCC__)
#define FQ_CAT_HD __host__ __device__ __forceinline__
#else
#define FQ_CAT_HD inline
#endif

namespace fq {

constexpr int kCatBlock = 256;         // threads per workgroup
constexpr int kCatMaxBlocks = 2048;    // 256 CUs x 8 workgroups: the lanes walk the rest of the pixels

struct CatSrcGeom {
    int C, Cpad;                       // real / stored channels of the source
    int lu;                            // log2 of the nearest-upsampling factor (0, 1, 2), alike on both axes
    int base;                          // first output channel of the source
};

template <int MAXSRC>
struct CatGeom {
    int nsrc;
    CatSrcGeom s[MAXSRC];              // entries at and behind nsrc: C = 0 (nothing of them lies in any chunk)
    int N, H, W;                       // OUTPUT plane; source i is [N][H >> lu][W >> lu][Cpad]
    int Cpad_out, CH;                  // CH = Cpad_out / 16
    unsigned npix;                     // N * H * W
};

// What source i contributes to the chunk k of every pixel.
struct CatPart {
    int use;                           // 0: nothing of this source lies in the chunk
    int s;                             // byte offset of the chunk's channel 0 in the source's pixel row (may be negative)
    int a, sh;                         // a = s rounded down to a dword, sh = s - a: dword t of the chunk = alignbyte(d[t + 1], d[t], sh)
    int lo, hi;                        // bytes [lo, hi) of the chunk come from this source
    unsigned ld;                       // bit t: the dword at row + a + 4t holds a wanted byte and is loaded (t = 0 .. 4)
    int whole16;                       // the 16 bytes at row + s are the chunk (s % 16 == 0, lo == 0; hi < 16 only masks the tail)
};

template <int MAXSRC>
FQ_CAT_HD CatPart cat_part(const CatGeom<MAXSRC>& g, int k, int i) {
    CatPart p;
    const int C = g.s[i].C;
    p.s = 16 * k - g.s[i].base;
    p.lo = p.s < 0 ? -p.s : 0;
    p.hi = C - p.s < 16 ? C - p.s : 16;
    p.use = i < g.nsrc && p.lo < p.hi;
    p.a = p.s & ~3;
    p.sh = p.s & 3;
    p.ld = 0u;
    p.whole16 = 0;
    if (!p.use) return p;
    for (int t = 0; t < 5; ++t) {
        const int o = p.a + 4 * t;                          // wanted bytes of the row: [s + lo, s + hi), inside [0, C)
        if (o < p.s + p.hi && o + 4 > p.s + p.lo) p.ld |= 1u << t;
    }
    p.whole16 = p.lo == 0 && (p.s & 15) == 0;
    return p;
}

// byte mask of dword t of the chunk for a part that owns the chunk's bytes [lo, hi)
FQ_CAT_HD unsigned cat_dword_mask(int lo, int hi, int t) {
    int l = lo - 4 * t, h = hi - 4 * t;
    l = l < 0 ? 0 : (l > 4 ? 4 : l);
    h = h < 0 ? 0 : (h > 4 ? 4 : h);
    if (l >= h) return 0u;
    const unsigned below_h = h == 4 ? 0xffffffffu : (1u << (8 * h)) - 1u;
    const unsigned below_l = (1u << (8 * l)) - 1u;          // l <= 3 here
    return below_h & ~below_l;
}

// pixel index of a source upsampled by 2^lu under the output pixel (n, h, w)
template <int MAXSRC>
FQ_CAT_HD unsigned cat_src_pix(const CatGeom<MAXSRC>& g, int lu, unsigned n, unsigned h, unsigned w) {
    return (n * ((unsigned)g.H >> lu) + (h >> lu)) * ((unsigned)g.W >> lu) + (w >> lu);
}

// every base_i % 16 == 0: each chunk is 16 bytes of exactly one source at a 16-byte-aligned offset (the aligned family)
template <int MAXSRC>
FQ_CAT_HD bool cat_aligned(const CatGeom<MAXSRC>& g) {
    bool a = true;
    for (int i = 0; i < MAXSRC; ++i) a = a && (i >= g.nsrc || (g.s[i].base & 15) == 0);
    return a;
}

// number of sources with a byte in chunk k
template <int MAXSRC>
FQ_CAT_HD int cat_owners(const CatGeom<MAXSRC>& g, int k) {
    int n = 0;
    for (int i = 0; i < MAXSRC; ++i) n += cat_part(g, k, i).use;
    return n;
}

// The chunk is one 16-byte load of source i: nobody else has a byte in it and it starts on a 16-byte boundary of the source's
// row (hi < 16 only behind the last source: the tail mask).  Both families take this path for such a chunk.
template <int MAXSRC>
FQ_CAT_HD bool cat_one16(const CatGeom<MAXSRC>& g, int k, int i) {
    const CatPart p = cat_part(g, k, i);
    return p.use && p.whole16 && cat_owners(g, k) == 1;
}

// How the lanes that own chunk k build it (what tests ask the case list to cover): kCatAligned16 one 16-byte load, kCatDword
// aligned dwords (sh == 0) of one source, kCatByte byte-shifted dwords of one source, kCatStraddle bytes of two or more sources.
enum CatClass { kCatAligned16 = 0, kCatDword = 1, kCatByte = 2, kCatStraddle = 3 };
template <int MAXSRC>
FQ_CAT_HD int cat_chunk_class(const CatGeom<MAXSRC>& g, int k) {
    if (cat_owners(g, k) > 1) return kCatStraddle;
    for (int i = 0; i < MAXSRC; ++i) {
        const CatPart p = cat_part(g, k, i);
        if (p.use) return p.whole16 ? kCatAligned16 : (p.sh == 0 ? kCatDword : kCatByte);
    }
    return kCatAligned16;                                   // (not reached: Cpad_out == pad16(sum C), every chunk has an owner)
}

// The launch: lane gid owns chunk k = gid % CH of the pixels gid / CH, + stride, + 2 stride, ... with stride = threads / CH;
// lanes whose first pixel is >= stride do nothing (they would repeat another lane's pixels).
template <int MAXSRC>
FQ_CAT_HD long cat_blocks(const CatGeom<MAXSRC>& g) {
    long b = ((long)g.npix * g.CH + kCatBlock - 1) / kCatBlock;
    return b > kCatMaxBlocks ? kCatMaxBlocks : b;
}

}  // namespace fq
