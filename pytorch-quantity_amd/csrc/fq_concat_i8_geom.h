// fq_concat_i8_geom.h -- the lane -> (sources, offsets, masks, loads) arithmetic, the host guards and the re-quantisation of the int8
// NHWC concatenations (fq_concat_i8.hip: the moving entry points fq_concat_i8_nhwc / fq_concat_n_i8_nhwc and the re-quantising
// fq_concat_rq_i8_nhwc), kept apart from the kernel so that the same functions compile as host code: scripts/concat_geom_check.cpp
// walks them over the shapes the GPU tests and the models run and asserts that every load lies inside its source and is aligned,
// that every output chunk is written exactly once, that the re-quantisation is v * 2^shift rounded half to even for every int8 and
// int16 value, and that the guards answer what include/fq.h says.
//
// The output is [N][H][W][Cpad_out] bytes; a CHUNK is 16 consecutive channels of one pixel (one dwordx4 store), CH = Cpad_out / 16
// chunks per pixel.  Chunk k holds output channels [16k, 16k + 16).  Source i owns output channels [base_i, base_i + C_i),
// base_i = C_0 + ... + C_{i-1}.  A source stores ELEMENTS of eb = 1 or 2 bytes (the moving kernels: always 1): everything below
// counts channels, and a byte offset is the channel offset times eb.  Relative to the source's pixel row the chunk starts at
// channel s = 16k - base_i (negative when the chunk begins in a source before), so one chunk may hold elements of every source.
// A lane keeps k for its whole life, so everything below except the pixel is per-lane constant.
//
// The geometry is a template on MAXSRC, the number of source entries of the kernel's parameter block: the moving kernel is
// instantiated at 2 (fq_concat_i8_nhwc) and at 8 (fq_concat_n_i8_nhwc), the re-quantising one at 8, and the two-source launch
// carries two entries, not eight.
#pragma once

#if defined(__HIPCC__)
#define FQ_CAT_HD __host__ __device__ __forceinline__
#else
#define FQ_CAT_HD inline
#endif

namespace fq {

constexpr int kCatBlock = 256;                   // threads per workgroup
constexpr int kCatMaxBlocks = 2048;              // 256 CUs x 8 workgroups: the lanes walk the rest of the pixels
constexpr int kCrqMaxSrc = 8;                    // FQ_CONCAT_N_MAX_SRC
constexpr int kCrqMaxShift = 8;                  // |b - g| of the re-quantising entry point
constexpr long kCrqMaxBytes = 0x7ffffffeL;       // the output and every source of every entry point: below 2^31 - 1 bytes

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

// ---------------------------------------------------------------- the host guards of all three entry points
FQ_CAT_HD int cat_log2_up(int up) { return up == 1 ? 0 : (up == 2 ? 1 : (up == 4 ? 2 : -1)); }

// What the *_supported predicates answer: channel counts, factors and, where the entry point has them (else null), element
// sizes and shifts.
FQ_CAT_HD bool cat_supported(const int* C, const int* up, const int* bytes, const int* shift, int nsrc, int maxsrc) {
    if (!C || !up || nsrc < 1 || nsrc > maxsrc) return false;
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (C[i] < 1 || C[i] > 65536 || cat_log2_up(up[i]) < 0 || (bytes && bytes[i] != 1 && bytes[i] != 2)) return false;
        if (shift && (shift[i] < -kCrqMaxShift || shift[i] > kCrqMaxShift)) return false;
        sum += C[i];
    }
    return sum <= 65536;                                   // the chunks of one pixel fit the smallest launch
}

// a * b * c * d > limit, each factor positive and below 2^31, without leaving long
FQ_CAT_HD bool cat_over(long a, long b, long c, long d, long limit) {
    long n = a;
    if (n > limit) return true;
    n *= b;
    if (n > limit) return true;
    n *= c;
    if (n > limit) return true;
    n *= d;
    return n > limit;
}

// Status of a call: 0 fine, -1 FQ_ERR_INVALID_ARG, -4 FQ_ERR_UNSUPPORTED, in the order include/fq.h gives.  `bytes` and `shift` are
// null for the moving entry points (every element one byte, every shift 0).  N == 0 is fine whatever the pointers and the other
// sizes are (nothing is launched).  The moving entry points judge their pointers between N == 0 and the sizes and pass the
// verdict in as bad_ptrs; the re-quantising one judges every scalar first, passes false and looks at its pointers afterwards.
FQ_CAT_HD int cat_args(const int* bytes, const int* C, const int* Cpad, const int* up, const int* relu, const int* shift, int nsrc,
                       int maxsrc, int Cpad_out, int N, int H, int W, bool bad_ptrs = false) {
    if (nsrc < 1 || N < 0 || H <= 0 || W <= 0) return -1;
    if (nsrc > maxsrc) return -4;
    long sum = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (C[i] < 1 || up[i] < 1 || Cpad[i] < C[i] || (relu[i] != 0 && relu[i] != 1)) return -1;
        if (bytes && bytes[i] != 1 && bytes[i] != 2) return -1;
        sum += C[i];
    }
    if (!cat_supported(C, up, bytes, shift, nsrc, maxsrc)) return -4;
    for (int i = 0; i < nsrc; ++i)
        if (Cpad[i] % 16 || H % up[i] || W % up[i]) return -4;
    if (Cpad_out != (int)((sum + 15) / 16 * 16)) return -1;
    if (nsrc == 1 && up[0] == 1 && !relu[0] && (!bytes || bytes[0] == 1) && (!shift || shift[0] == 0)) return -1;      // nothing to do
    if (N == 0) return 0;
    if (bad_ptrs) return -1;
    if (cat_over(N, H, W, Cpad_out, kCrqMaxBytes)) return -4;
    for (int i = 0; i < nsrc; ++i)
        if (cat_over(N, H / up[i], W / up[i], (long)Cpad[i] * (bytes ? bytes[i] : 1), kCrqMaxBytes)) return -4;
    return 0;
}

// the geometry of a call that cat_args admits
template <int MAXSRC>
FQ_CAT_HD CatGeom<MAXSRC> cat_geom(const int* C, const int* Cpad, const int* up, int nsrc, int Cpad_out, int N, int H, int W) {
    CatGeom<MAXSRC> g;
    g.nsrc = nsrc;
    int base = 0;
    for (int i = 0; i < MAXSRC; ++i) {
        const bool have = i < nsrc;
        g.s[i].C = have ? C[i] : 0;
        g.s[i].Cpad = have ? Cpad[i] : 16;
        g.s[i].lu = have ? cat_log2_up(up[i]) : 0;
        g.s[i].base = base;
        base += g.s[i].C;
    }
    g.N = N; g.H = H; g.W = W; g.Cpad_out = Cpad_out; g.CH = Cpad_out / 16;
    g.npix = (unsigned)((long)N * H * W);
    return g;
}

// ---------------------------------------------------------------- what a lane does
// What source i contributes to the chunk k of every pixel.
struct CatPart {
    int use;                           // 0: nothing of this source lies in the chunk
    int s;                             // channel of the source's pixel row at the chunk's channel 0 (may be negative)
    int lo, hi;                        // channels [lo, hi) of the chunk come from this source
    int whole16;                       // the 16 elements at row + s are the chunk (s % 16 == 0, lo == 0; hi < 16 only masks the tail)
    // the general family: the chunk's elements start at byte s * eb of the row; a = that rounded down to a dword, sh = the rest
    // (int8: 0 .. 3, int16: 0 or 2); dword t of the elements = alignbyte(d[t + 1], d[t], sh), t < 4 (int8) or t < 8 (int16)
    int a, sh;
    unsigned ld;                       // bit t: the dword at row + a + 4t holds a wanted byte and is loaded (t = 0 .. 4, or 0 .. 8)
};

// eb: the element size of source i in bytes, 1 or 2
template <int MAXSRC>
FQ_CAT_HD CatPart cat_part(const CatGeom<MAXSRC>& g, int k, int i, int eb) {
    CatPart p;
    const int C = g.s[i].C;
    p.s = 16 * k - g.s[i].base;
    p.lo = p.s < 0 ? -p.s : 0;
    p.hi = C - p.s < 16 ? C - p.s : 16;
    p.use = i < g.nsrc && p.lo < p.hi;
    p.a = (p.s * eb) & ~3;
    p.sh = (p.s * eb) & 3;
    p.ld = 0u;
    p.whole16 = 0;
    if (!p.use) return p;
    for (int t = 0; t < 4 * eb + 1; ++t) {
        const int o = p.a + 4 * t;                          // wanted bytes of the row: [(s + lo) eb, (s + hi) eb), inside [0, C eb)
        if (o < (p.s + p.hi) * eb && o + 4 > (p.s + p.lo) * eb) p.ld |= 1u << t;
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

// every base_i % 16 == 0: each chunk is 16 elements of exactly one source at a 16-element-aligned offset (the aligned family)
template <int MAXSRC>
FQ_CAT_HD bool cat_aligned(const CatGeom<MAXSRC>& g) {
    bool a = true;
    for (int i = 0; i < MAXSRC; ++i) a = a && (i >= g.nsrc || (g.s[i].base & 15) == 0);
    return a;
}

template <int MAXSRC>
FQ_CAT_HD bool cat_upsampled(const CatGeom<MAXSRC>& g) {
    bool u = false;
    for (int i = 0; i < MAXSRC; ++i) u = u || g.s[i].lu > 0;
    return u;
}

// number of sources with an element in chunk k (use, lo, hi, s and whole16 do not depend on the element size)
template <int MAXSRC>
FQ_CAT_HD int cat_owners(const CatGeom<MAXSRC>& g, int k) {
    int n = 0;
    for (int i = 0; i < MAXSRC; ++i) n += cat_part(g, k, i, 1).use;
    return n;
}

// The chunk is one 16-element load of source i: nobody else has an element in it and it starts on a 16-element boundary of the
// source's row (hi < 16 only behind the last source: the tail mask).  Both families take this path for such a chunk.
template <int MAXSRC>
FQ_CAT_HD bool cat_one16(const CatGeom<MAXSRC>& g, int k, int i) {
    const CatPart p = cat_part(g, k, i, 1);
    return p.use && p.whole16 && cat_owners(g, k) == 1;
}

// How the lanes that own chunk k build it from one-byte elements (what tests ask the case list to cover): kCatAligned16 one 16-byte
// load, kCatDword aligned dwords (sh == 0) of one source, kCatByte byte-shifted dwords of one source, kCatStraddle bytes of two
// or more sources.
enum CatClass { kCatAligned16 = 0, kCatDword = 1, kCatByte = 2, kCatStraddle = 3 };
template <int MAXSRC>
FQ_CAT_HD int cat_chunk_class(const CatGeom<MAXSRC>& g, int k) {
    if (cat_owners(g, k) > 1) return kCatStraddle;
    for (int i = 0; i < MAXSRC; ++i) {
        const CatPart p = cat_part(g, k, i, 1);
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

// ---------------------------------------------------------------- the rounding rule of the re-quantising entry point
// r = v * 2^shift rounded half to even, then the ReLU and the clamp to int8, as shift amounts and masks (crq_requant)
struct CrqRound {
    int rsh, lsh;                      // shift < 0: rsh = -shift; shift > 0: lsh = shift
    int mask;                          // 2^rsh - 1: the bits the right shift drops
    int bias;                          // 2^(rsh - 1) - 1 (0 for rsh == 0)
    int odd;                           // 1 where rsh > 0: the bit of the quotient that decides a tie
    int lo;                            // 0 with the ReLU, else -128
};

FQ_CAT_HD CrqRound crq_round(int shift, int relu) {
    CrqRound r;
    r.rsh = shift < 0 ? -shift : 0;
    r.lsh = shift > 0 ? shift : 0;
    r.mask = (1 << r.rsh) - 1;
    r.bias = r.rsh > 0 ? (1 << (r.rsh - 1)) - 1 : 0;
    r.odd = r.rsh > 0 ? 1 : 0;
    r.lo = relu ? 0 : -128;
    return r;
}

// The rule on one int8 or int16 value, in plain integers; the kernel does the same steps on packed int16, so every intermediate
// has to fit int16 for EVERY int16 v (the walker asserts it through `fits`):
//   q = v >> rsh (floor), rem = v & mask;  rem + bias + 1 <= 255 + 127 + 1;  q + 1 <= 2^14 + 1 for rsh >= 1 -- the rounding addend
//   never meets v itself, so nothing wraps at |v| near 2^15; for rsh == 0 the addend is 0 and q = v;
//   half to even: the dropped bits plus 2^(rsh-1) - 1 plus the quotient's lowest bit carry into bit rsh exactly when the value
//   rounds up;
//   the clamp to [lo, 127] BEFORE the left shift (monotone, so the result is unchanged) keeps 127 * 2^8 = 32512 inside int16,
//   the clamp after it is the rule's own.
FQ_CAT_HD bool crq_fits16(int x) { return x >= -32768 && x <= 32767; }

FQ_CAT_HD int crq_requant(int v, const CrqRound& r, bool* fits = nullptr) {
    const int q = v >> r.rsh;
    const int a = (v & r.mask) + r.bias + (q & r.odd);
    int x = q + (a >> r.rsh);
    bool ok = crq_fits16(a) && crq_fits16(x);
    x = x < r.lo ? r.lo : (x > 127 ? 127 : x);
    x = x * (1 << r.lsh);
    ok = ok && crq_fits16(x);
    if (fits) *fits = ok;
    return x < r.lo ? r.lo : (x > 127 ? 127 : x);
}

}  // namespace fq
