// Host check of the concat kernel's address arithmetic, rounding and guards (csrc/fq_concat_i8_geom.h), for both element policies
// of the kernel and every instantiation (moving at MAXSRC = 2: fq_concat_i8_nhwc, at 8: fq_concat_n_i8_nhwc; re-quantising at 8:
// fq_concat_rq_i8_nhwc): every lane of every launch loads inside its source (aligned, a dword or 16 bytes), assembles exactly the
// elements the index rule asks for, every output chunk is written exactly once, an aligned launch is made of 16-byte loads only;
// the re-quantisation is v * 2^shift rounded half to even in double for all 256 int8 and all 65 536 int16 values, every shift in
// [-8, 8] and both ReLU flags, with every packed-int16 intermediate inside int16; the host guards answer the return codes of
// include/fq.h for all three entry points.
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o concat_geom_check scripts/concat_geom_check.cpp
//   ./concat_geom_check                                          the built-in shape lists of both policies (moving: cases of one or
//                                                                two sources at both limits, the rest at 8), the rounding, the guards
//   ./concat_geom_check N,H,W/C0,C1,.../up0,up1,... ...           these cases as the moving kernel walks them
//   ./concat_geom_check N,H,W/C0,.../up0,.../bytes0,... ...       ... as the re-quantising kernel does (bytes: 1 int8, 2 int16), source
//                                                                i with relu = i & 1 and shift = (5 i) % 17 - 8; then the rounding
//                                                                and the guards.  Tests pass the GPU tests' and the models' lists
//   ./concat_geom_check maxsrc=2|8 <cases>                       the moving instantiation whose geometry is walked (default 8); a case
//                                                                with more sources is an error
//   ./concat_geom_check window=P <cases>                         a size-limit row (10^8 chunks): only the first and the last P pixels
//                                                                of the output are walked, by the lanes and in the order the kernel
//                                                                visits them; no tensor reaches 2^31 bytes, so there is no boundary between
// One line per case given: "case N,H,W/C.../up...: aligned16 A dword D byte B straddle S" (chunks of one pixel by cat_chunk_class) or
// "case N,H,W/C.../up.../bytes...: aligned16 A general G chunks X blocks B second-items S"; behind re-quantising cases "requant: V
// values, T ties" and "guards: G rows"; then "ok, <loads> loads checked".  Exit status 1 at the first violation, 2 for a case that
// cannot be read.
// The walk below is the kernel's own: same launch size, same lane -> (chunk, first pixel, stride), the same predicates in
// front of every load; the bytes are carried through the same shift-and-mask steps on a model of memory whose every byte is
// its own address, so that a wrong byte is seen as well as a wrong address.  (The ReLU and the rounding act on values, not on
// addresses: they are applied to each part in front of the or and have no place in this model; check_requant holds the rounding.)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_concat_i8_geom.h"

using namespace fq;

constexpr int kMaxSrc = 8;
struct Case { int N, H, W, nsrc, C[kMaxSrc], up[kMaxSrc], bytes[kMaxSrc]; bool requant; std::string text; };

static void fail(const char* what, const std::string& where) {
    printf("%s: %s\n", what, where.c_str());
    exit(1);
}

static std::string list_of(const int* v, int n) {
    std::string s;
    for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

static std::string text_of(const Case& c) {
    return std::to_string(c.N) + "," + std::to_string(c.H) + "," + std::to_string(c.W) + "/" + list_of(c.C, c.nsrc) + "/" +
           list_of(c.up, c.nsrc) + (c.requant ? "/" + list_of(c.bytes, c.nsrc) : "");
}

// v_alignbyte_b32: ({hi, lo} >> 8 * sh) & 0xffffffff on "addresses" instead of bytes: byte j of the result is byte sh + j of the
// pair; -2 marks a byte of a dword that was not loaded
static void alignbyte(const long (&hi)[4], const long (&lo)[4], int sh, long (&out)[4]) {
    for (int j = 0; j < 4; ++j) out[j] = sh + j < 4 ? lo[sh + j] : hi[sh + j - 4];
}

static unsigned long g_window = 0;          // window=P: pixels [P, npix - P) are skipped

// One launch of concat_kernel<ELEM, MAXSRC, ., .>: ELEM = CatRequant where c.requant (element sizes c.bytes), else CatMove.
template <int MAXSRC>
static long run(const Case& c, bool print) {
    if (c.nsrc > MAXSRC) fail("more sources than maxsrc", c.text);
    const bool rq = c.requant;
    int Cpad[MAXSRC], relu[MAXSRC], shift[MAXSRC], wide[MAXSRC];
    long sum = 0;
    for (int i = 0; i < MAXSRC; ++i) wide[i] = 0;
    for (int i = 0; i < c.nsrc; ++i) {
        if (!rq && (c.C[i] < 1 || (c.up[i] != 1 && c.up[i] != 2 && c.up[i] != 4))) fail("bad channel count or factor", c.text);
        if (!rq && (c.H % c.up[i] || c.W % c.up[i])) fail("plane is no multiple of the factor", c.text);
        Cpad[i] = (c.C[i] + 15) / 16 * 16;
        relu[i] = rq ? i & 1 : 1;                          // (moving: a ReLU everywhere, so that one plain source is work)
        shift[i] = rq ? (i * 5) % 17 - 8 : 0;
        wide[i] = c.bytes[i] == 2;                          // CatRequant::src
        sum += c.C[i];
    }
    const int Cpad_out = (int)((sum + 15) / 16 * 16);
    if (cat_args(rq ? c.bytes : nullptr, c.C, Cpad, c.up, relu, rq ? shift : nullptr, c.nsrc, MAXSRC, Cpad_out, c.N, c.H, c.W) != 0)
        fail("the guards refuse the case", c.text);
    const CatGeom<MAXSRC> g = cat_geom<MAXSRC>(c.C, Cpad, c.up, c.nsrc, Cpad_out, c.N, c.H, c.W);
    long src_bytes[MAXSRC];
    for (int i = 0; i < MAXSRC; ++i)
        src_bytes[i] = i < c.nsrc ? (long)c.N * (c.H / c.up[i]) * (c.W / c.up[i]) * Cpad[i] * c.bytes[i] : 0;
    const bool general = !cat_aligned(g);
    int cls[4] = {0, 0, 0, 0};
    for (int k = 0; k < g.CH; ++k) ++cls[cat_chunk_class(g, k)];
    if (!rq && !general && (cls[kCatDword] || cls[kCatByte] || cls[kCatStraddle]))
        fail("an aligned launch holds a chunk that is not one 16-byte load", c.text);

    const unsigned threads = (unsigned)cat_blocks(g) * kCatBlock, stride = threads / g.CH;
    // the kernel's pixel index, lane number and `pix += stride` are 32 bits wide
    if ((unsigned long)g.npix + stride > 0xffffffffUL || (unsigned long)g.npix * g.CH > 0xffffffffUL) fail("32-bit pixel arithmetic wraps", c.text);
    const bool windowed = g_window && (unsigned long)g.npix > 2 * g_window;
    const unsigned long walked = windowed ? 2 * g_window : g.npix;
    auto slot = [&](unsigned pix) { return !windowed || pix < g_window ? (size_t)pix : (size_t)(g_window + (pix - (g.npix - g_window))); };
    std::vector<unsigned char> written((size_t)walked * g.CH, 0);
    long loads = 0, second = 0;
    int n16 = 0, ngen = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int k = gid % g.CH;
        unsigned pix = gid / g.CH;
        if (pix >= stride) continue;
        CatPart part[MAXSRC];
        int owners = 0, whole = 0;
        for (int i = 0; i < MAXSRC; ++i) {
            part[i] = cat_part(g, k, i, wide[i] ? 2 : 1);
            owners += part[i].use;
            whole |= part[i].use & part[i].whole16;
        }
        const bool one16 = owners == 1 && whole;            // the kernel's test in front of cat_loop16
        if (!general && !one16) fail(rq ? "aligned launch: the chunk is not 16 elements of one source" : "aligned launch: the chunk is not 16 bytes of one source", c.text);
        for (int i = 0; i < MAXSRC; ++i)
            if (one16 != cat_one16(g, k, i) && part[i].use) fail("cat_one16 disagrees with the kernel's test", c.text);
        if (pix == 0) ++(one16 ? n16 : ngen);
        const unsigned first = pix;
        for (; pix < g.npix; pix += stride) {
            if (windowed && pix >= g_window && pix < g.npix - g_window) {      // jump to this lane's first pixel of the last window
                const unsigned long steps = ((unsigned long)(g.npix - g_window) - pix + stride - 1) / stride;
                const unsigned long next = pix + steps * stride;
                if (next >= g.npix) break;
                pix = (unsigned)(next - stride);
                continue;
            }
            if (pix != first) ++second;
            const unsigned w = pix % g.W, h = (pix / g.W) % g.H, n = pix / g.W / g.H;
            // the elements the kernel assembles, as (source, address of the first byte) pairs; got[j] = -1: zero
            long got[16];
            int got_src[16];
            for (int j = 0; j < 16; ++j) { got[j] = -1; got_src[j] = -1; }
            for (int i = 0; i < MAXSRC; ++i) {
                const CatPart& p = part[i];
                if (!(i < g.nsrc) || !p.use) continue;
                if (!one16 && !p.ld) fail("a used part loads nothing", c.text);
                const int eb = wide[i] ? 2 : 1;             // CatRequant::bytes
                if (eb != c.bytes[i]) fail("element size", c.text);
                const unsigned sp = cat_src_pix(g, g.s[i].lu, n, h, w);
                if (g.s[i].lu == 0 && sp != pix) fail("source pixel of a source that is not upsampled", c.text);
                const long rowbytes = (long)g.s[i].Cpad * eb, row = (long)sp * rowbytes;
                long bytes[32];
                if (one16) {
                    for (int l = 0; l < eb; ++l) {
                        const long in_row = (long)p.s * eb + 16 * l, o = row + in_row;
                        if (o < 0 || o % 16 || o + 16 > src_bytes[i]) fail("16-byte load outside its source or unaligned", c.text);
                        if (in_row < 0 || in_row + 16 > rowbytes) fail("16-byte load outside its pixel row", c.text);
                        ++loads;
                        for (int j = 0; j < 16; ++j) bytes[16 * l + j] = o + j;
                    }
                } else {
                    long d[9][4];
                    for (int t = 0; t < 4 * eb + 1; ++t) {
                        for (int j = 0; j < 4; ++j) d[t][j] = -2;                   // not loaded: zero in the kernel
                        if (!(p.ld & (1u << t))) continue;
                        const long o = row + p.a + 4 * t;
                        if (o < 0 || o % 4 || o + 4 > src_bytes[i]) fail("dword load outside its source or unaligned", c.text);
                        if (p.a + 4 * t < 0 || p.a + 4 * t + 4 > rowbytes) fail("dword load outside its pixel row", c.text);
                        ++loads;
                        for (int j = 0; j < 4; ++j) d[t][j] = o + j;
                    }
                    if (p.ld >> (4 * eb + 1)) fail("a load bit past the part's dwords", c.text);
                    if (eb == 2 && (p.sh & 1)) fail("an int16 part at an odd byte", c.text);
                    for (int t = 0; t < 4 * eb; ++t) {
                        long o4[4];
                        alignbyte(d[t + 1], d[t], p.sh, o4);
                        for (int j = 0; j < 4; ++j) bytes[4 * t + j] = o4[j];
                    }
                }
                for (int t = 0; t < 4; ++t) {
                    const unsigned m = cat_dword_mask(one16 ? 0 : p.lo, p.hi, t);
                    for (int j = 0; j < 4; ++j) {
                        if (!((m >> (8 * j)) & 0xffu)) continue;
                        if (((m >> (8 * j)) & 0xffu) != 0xffu) fail("partial byte mask", c.text);
                        const int el = 4 * t + j;
                        if (got[el] != -1) fail("two sources write one output byte", c.text);
                        if (bytes[el * eb] < 0) fail("a wanted byte comes from a dword that was not loaded", c.text);
                        if (eb == 2 && (bytes[el * eb] % 2 || bytes[el * eb + 1] != bytes[el * eb] + 1)) fail("an int16 element is torn", c.text);
                        got[el] = bytes[el * eb];
                        got_src[el] = i;
                    }
                }
            }
            for (int j = 0; j < 16; ++j) {                  // the index rule and the channel mask
                const int ch = 16 * k + j;
                int i = -1;
                for (int q = 0; q < c.nsrc; ++q)
                    if (ch >= g.s[q].base && ch < g.s[q].base + c.C[q]) i = q;
                long want = -1;
                if (i >= 0) {
                    const int u = c.up[i];
                    want = ((((long)n * (c.H / u) + h / u) * (c.W / u) + w / u) * g.s[i].Cpad + (ch - g.s[i].base)) * c.bytes[i];
                }
                if (got[j] != want || got_src[j] != i)
                    fail(rq ? "output byte is not the element the index rule names" : "output byte is not the byte the index rule names", c.text);
            }
            if (((size_t)pix * g.CH + k + 1) * 16 > (size_t)g.npix * g.Cpad_out) fail("store outside the output", c.text);
            if (written[slot(pix) * g.CH + k]++) fail("output chunk written twice", c.text);
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output chunk not written", c.text);
    if (print && rq)
        printf("case %s: aligned16 %d general %d chunks %lu blocks %ld second-items %ld\n", c.text.c_str(), n16, ngen,
               (unsigned long)g.npix * g.CH, cat_blocks(g), second);
    else if (print)
        printf("case %s: aligned16 %d dword %d byte %d straddle %d\n", c.text.c_str(), cls[0], cls[1], cls[2], cls[3]);
    return loads;
}

static std::string check_requant() {
    long values = 0, ties = 0;
    for (int shift = -kCrqMaxShift; shift <= kCrqMaxShift; ++shift)
        for (int relu = 0; relu < 2; ++relu) {
            const CrqRound r = crq_round(shift, relu);
            const std::string where = "shift " + std::to_string(shift) + " relu " + std::to_string(relu);
            for (int v = -32768; v <= 32767; ++v) {
                const double exact = std::ldexp((double)v, shift);
                double want = std::nearbyint(exact);                           // round half to even (the default rounding mode)
                if (exact - std::floor(exact) == 0.5) ++ties;
                if (relu && want < 0) want = 0;
                want = want < -128 ? -128 : (want > 127 ? 127 : want);
                bool fits = false;
                if (crq_requant(v, r, &fits) != (int)want) fail("re-quantisation differs from rint(v * 2^shift)", where + " v " + std::to_string(v));
                if (!fits) fail("an intermediate leaves int16", where + " v " + std::to_string(v));
                ++values;
            }
        }
    return "requant: " + std::to_string(values) + " values (int8 is the range [-128, 127] of them), " + std::to_string(ties) + " ties";
}

// The statuses of include/fq.h, by cat_args as each entry point calls it: maxsrc 0 stands for fq_concat_rq_i8_nhwc (bytes and shift
// passed, the pointers judged behind the scalars), 2 for fq_concat_i8_nhwc and 8 for fq_concat_n_i8_nhwc (neither passed, a bad
// pointer judged between N == 0 and the sizes).
static std::string check_guards() {
    const int INV = -1, UNS = -4;
    struct Row { int want; int maxsrc; int nsrc; int bytes[2], C[2], Cpad[2], up[2], relu[2], shift[2]; int Cpad_out, N, H, W; bool bad_ptrs; const char* what; };
    const Row rows[] = {
        {0, 0, 2, {1, 2}, {16, 16}, {16, 16}, {1, 1}, {0, 1}, {-3, 2}, 32, 2, 4, 4, false, "a plain call"},
        {0, 0, 1, {2, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {0, 0}, 16, 1, 4, 4, false, "one int16 source at shift 0 is work"},
        {0, 0, 1, {1, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {1, 0}, 16, 1, 4, 4, false, "one int8 source at shift 1 is work"},
        {INV, 0, 1, {1, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {0, 0}, 16, 1, 4, 4, false, "nothing to do"},
        {INV, 0, 0, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 0}, 32, 1, 4, 4, false, "no source"},
        {UNS, 0, 9, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 0}, 32, 1, 4, 4, false, "nine sources"},
        {INV, 0, 2, {1, 3}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, false, "bytes 3"},
        {INV, 0, 2, {0, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, false, "bytes 0"},
        {INV, 0, 2, {1, 1}, {0, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 16, 1, 4, 4, false, "C 0"},
        {INV, 0, 2, {1, 1}, {17, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 48, 1, 4, 4, false, "Cpad < C"},
        {INV, 0, 2, {1, 1}, {16, 16}, {16, 16}, {0, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, false, "up 0"},
        {INV, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {2, 0}, {0, 1}, 32, 1, 4, 4, false, "relu 2"},
        {INV, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 48, 1, 4, 4, false, "Cpad_out"},
        {INV, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, -1, 4, 4, false, "N < 0"},
        {INV, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 0, 4, false, "H 0"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 9}, 32, 1, 4, 4, false, "shift 9"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {-9, 0}, 32, 1, 4, 4, false, "shift -9"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {3, 1}, {0, 0}, {0, 1}, 32, 1, 6, 6, false, "up 3"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {2, 1}, {0, 0}, {0, 1}, 32, 1, 5, 4, false, "H % up"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {24, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, false, "Cpad % 16"},
        {UNS, 0, 2, {1, 1}, {65536, 16}, {65536, 16}, {1, 1}, {0, 0}, {0, 1}, 65552, 1, 4, 4, false, "sum C > 65536"},
        {0, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 0, 1 << 30, 1 << 30, false, "N == 0"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 8192, 8192, false, "an output of 2^31 bytes"},
        {0, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 8192, 8191, false, "an output just under the limit"},
        {UNS, 0, 2, {1, 2}, {1, 16}, {16, 1024}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 1024, 1024, false, "an int16 source of 2^31 bytes"},
        {0, 0, 2, {1, 1}, {1, 16}, {16, 1024}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 1024, 1024, false, "... that fits as int8"},
        {UNS, 0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1 << 30, 1 << 30, 1 << 30, false, "sizes whose product leaves long"},
        // the moving entry points: fq_concat_i8_nhwc (one ReLU flag for the call, in both entries) and fq_concat_n_i8_nhwc
        {0, 2, 2, {}, {16, 16}, {16, 16}, {1, 2}, {1, 1}, {}, 32, 2, 4, 4, false, "two sources: a plain call"},
        {0, 8, 2, {}, {20, 44}, {32, 48}, {2, 1}, {0, 1}, {}, 64, 2, 4, 4, false, "N sources: a plain call"},
        {INV, 2, 1, {}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {}, 16, 1, 4, 4, false, "two sources: nothing to do"},
        {INV, 8, 1, {}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {}, 16, 1, 4, 4, false, "N sources: nothing to do"},
        {0, 2, 1, {}, {16, 0}, {16, 0}, {1, 0}, {1, 0}, {}, 16, 1, 4, 4, false, "one source with a ReLU is work"},
        {0, 8, 1, {}, {16, 0}, {16, 0}, {2, 0}, {0, 0}, {}, 16, 1, 4, 4, false, "one upsampled source is work"},
        {INV, 2, 0, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 1, 4, 4, false, "two sources: no source"},
        {UNS, 2, 3, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 48, 1, 4, 4, false, "two sources: three"},
        {UNS, 8, 9, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 144, 1, 4, 4, false, "N sources: nine"},
        {INV, 2, 2, {}, {0, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 16, 1, 4, 4, false, "two sources: C 0"},
        {INV, 8, 2, {}, {16, 16}, {16, 16}, {1, 0}, {0, 0}, {}, 32, 1, 4, 4, false, "N sources: up 0"},
        {INV, 2, 2, {}, {16, 17}, {16, 16}, {1, 1}, {0, 0}, {}, 48, 1, 4, 4, false, "two sources: Cpad < C"},
        {INV, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 2}, {}, 32, 1, 4, 4, false, "N sources: relu 2"},
        {INV, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {-1, 0}, {}, 32, 1, 4, 4, false, "N sources: relu -1"},
        {INV, 2, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 48, 1, 4, 4, false, "two sources: Cpad_out"},
        {INV, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, -1, 4, 4, false, "N sources: N < 0"},
        {INV, 2, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 1, 4, 0, false, "two sources: W 0"},
        {UNS, 2, 2, {}, {16, 16}, {16, 16}, {1, 8}, {0, 0}, {}, 32, 1, 8, 8, false, "two sources: up 8"},
        {UNS, 8, 2, {}, {16, 16}, {16, 16}, {1, 4}, {0, 0}, {}, 32, 1, 4, 6, false, "N sources: W % up"},
        {UNS, 8, 2, {}, {16, 16}, {16, 24}, {1, 1}, {0, 0}, {}, 32, 1, 4, 4, false, "N sources: Cpad % 16"},
        {UNS, 2, 2, {}, {65536, 1}, {65536, 16}, {1, 1}, {0, 0}, {}, 65552, 1, 1, 1, false, "two sources: sum C > 65536"},
        {INV, 8, 2, {}, {0, 16}, {16, 16}, {3, 1}, {0, 0}, {}, 16, 1, 4, 4, false, "an invalid argument is named before an unsupported one"},
        {INV, 2, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 1, 4, 4, true, "two sources: a null or misaligned pointer"},
        {INV, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 512, 256, 256, true, "N sources: a bad pointer is named before the sizes"},
        {0, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 0, 1 << 30, 1 << 30, true, "N sources: N == 0 whatever the pointers and sizes are"},
        {UNS, 8, 2, {}, {16, 16}, {16, 16}, {3, 1}, {0, 0}, {}, 32, 0, 6, 6, true, "N sources: N == 0 does not excuse another factor"},
        {UNS, 2, 2, {}, {32, 32}, {32, 32}, {1, 1}, {1, 1}, {}, 64, 512, 256, 256, false, "two sources: an output of 2^31 bytes"},
        {UNS, 8, 2, {}, {32, 32}, {32, 32}, {1, 1}, {0, 0}, {}, 64, 512, 256, 256, false, "N sources: an output of 2^31 bytes"},
        {UNS, 2, 2, {}, {1, 1}, {1024, 16}, {1, 1}, {1, 1}, {}, 16, 32, 256, 256, false, "two sources: a source of 2^31 bytes"},
        {UNS, 8, 2, {}, {1, 1}, {1024, 16}, {1, 1}, {0, 0}, {}, 16, 32, 256, 256, false, "N sources: a source of 2^31 bytes"},
        {0, 2, 2, {}, {20, 44}, {32, 48}, {2, 1}, {1, 1}, {}, 64, 520, 254, 254, false, "two sources: an output just under the limit"},
        {0, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 1, 8192, 8191, false, "N sources: an output just under the limit"},
        {UNS, 8, 2, {}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {}, 32, 1 << 30, 1 << 30, 1 << 30, false, "N sources: sizes whose product leaves long"},
    };
    int n = 0;
    for (const Row& r : rows) {
        const bool rq = r.maxsrc == 0;
        if (cat_args(rq ? r.bytes : nullptr, r.C, r.Cpad, r.up, r.relu, rq ? r.shift : nullptr, r.nsrc, rq ? kCrqMaxSrc : r.maxsrc, r.Cpad_out,
                     r.N, r.H, r.W, r.bad_ptrs) != r.want)
            fail("guard", r.what);
        ++n;
    }
    const int C[2] = {16, 16}, up[2] = {1, 4}, by[2] = {1, 2}, sh[2] = {-8, 8}, sh9[2] = {0, 9}, by3[2] = {1, 3}, C3[3] = {16, 16, 16}, up3[3] = {1, 1, 1};
    if (!cat_supported(C, up, by, sh, 2, 8) || cat_supported(C, up, by, sh9, 2, 8) || cat_supported(C, up, by3, sh, 2, 8) ||
        cat_supported(C, up, by, sh, 0, 8) || cat_supported(nullptr, up, by, sh, 2, 8))
        fail("guard", "cat_supported with element sizes and shifts");
    if (!cat_supported(C, up, nullptr, nullptr, 2, 2) || cat_supported(C3, up3, nullptr, nullptr, 3, 2) || !cat_supported(C3, up3, nullptr, nullptr, 3, 8) ||
        cat_supported(C, nullptr, nullptr, nullptr, 2, 8))
        fail("guard", "cat_supported");
    return "guards: " + std::to_string(n + 9) + " rows";
}

static bool parse_list(const std::string& s, int* out, int& n) {
    n = 0;
    const char* p = s.c_str();
    while (*p) {
        char* end;
        const long v = strtol(p, &end, 10);
        if (end == p || n >= kMaxSrc || (*end && *end != ',')) return false;
        out[n++] = (int)v;
        p = *end == ',' ? end + 1 : end;
    }
    return n > 0;
}

// N,H,W/C.../up... (the moving kernel) or N,H,W/C.../up.../bytes... (the re-quantising one)
static bool parse(const char* arg, Case& c) {
    std::vector<std::string> parts;
    std::string a(arg);
    size_t at = 0;
    for (;;) {
        const size_t p = a.find('/', at);
        parts.push_back(a.substr(at, p == std::string::npos ? p : p - at));
        if (p == std::string::npos) break;
        at = p + 1;
    }
    if ((parts.size() != 3 && parts.size() != 4) || sscanf(parts[0].c_str(), "%d,%d,%d", &c.N, &c.H, &c.W) != 3) return false;
    c.requant = parts.size() == 4;
    int nc = 0, nu = 0, nb = 0;
    if (!parse_list(parts[1], c.C, nc) || !parse_list(parts[2], c.up, nu) || nc != nu) return false;
    if (c.requant && (!parse_list(parts[3], c.bytes, nb) || nb != nc)) return false;
    for (int i = 0; i < nc && !c.requant; ++i) c.bytes[i] = 1;
    c.nsrc = nc;
    c.text = text_of(c);
    return c.N > 0 && c.H > 0 && c.W > 0;
}

// the moving kernel's case where `bytes` is empty; missing factors are 1
static Case make(int N, int H, int W, std::vector<int> C, std::vector<int> up, std::vector<int> bytes = {}) {
    Case c;
    c.N = N; c.H = H; c.W = W; c.nsrc = (int)C.size();
    c.requant = !bytes.empty();
    for (int i = 0; i < c.nsrc; ++i) {
        c.C[i] = C[i];
        c.up[i] = i < (int)up.size() ? up[i] : 1;
        c.bytes[i] = i < (int)bytes.size() ? bytes[i] : 1;
    }
    c.text = text_of(c);
    return c;
}

static std::vector<Case> builtin_moving() {
    std::vector<Case> cases;
    const int planes[][3] = {{1, 1, 1}, {2, 3, 5}, {1, 4, 4}, {3, 7, 9}, {2, 8, 12}};
    // one and two sources, every pair of factors
    const std::vector<std::vector<int>> two = {{16, 16}, {64, 64}, {20, 44}, {3, 5}, {17, 30}, {13, 3}, {1, 1}, {24, 8}, {5, 7}, {15, 1},
                                               {1, 15}, {31, 33}, {4, 12}, {100, 28}, {3}, {16}, {40}};
    for (const auto& ch : two)
        for (const auto& pl : planes)
            for (int u0 : {1, 2, 4})
                for (int u1 : {1, 2, 4}) {
                    if (pl[1] % u0 || pl[2] % u0 || pl[1] % u1 || pl[2] % u1 || (ch.size() == 1 && u1 != 1)) continue;
                    cases.push_back(make(pl[0], pl[1], pl[2], ch, {u0, u1}));
                }
    cases.push_back(make(64, 56, 56, {64, 64}, {}));                  // more chunks than the launch has lanes: the stride over pixels
    cases.push_back(make(16, 52, 52, {24, 100}, {1, 2}));
    // up to eight sources
    const std::vector<std::vector<int>> chans = {
        {16, 32, 16, 48}, {16, 16, 16, 16, 16, 16, 16, 16}, {20, 44, 13}, {17, 1, 30}, {3, 5, 1, 2, 4, 1, 7, 6}, {13, 2, 1},
        {1, 1, 1}, {24, 8, 16}, {5, 7, 9}, {8, 12, 8, 4}, {1, 1, 1, 1, 1, 1, 1, 1}, {15, 1, 16}, {16, 3, 13, 32}, {31, 33, 2},
        {4, 4, 4, 4, 16}, {100, 28, 7}, {16, 16}, {3, 5}, {40}, {3}};
    const std::vector<std::vector<int>> factors = {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 1, 4, 1, 2, 1, 4, 1}, {1, 2, 1, 4, 1, 2, 1, 4},
                                                   {4, 4, 2, 2, 1, 1, 2, 4}, {2, 2, 2, 2, 2, 2, 2, 2}};
    for (const auto& ch : chans)
        for (const auto& pl : planes)
            for (const auto& f : factors) {
                bool ok = true;
                std::vector<int> up(f.begin(), f.begin() + ch.size());
                for (int u : up) ok = ok && pl[1] % u == 0 && pl[2] % u == 0;
                if (ok) cases.push_back(make(pl[0], pl[1], pl[2], ch, up));
            }
    cases.push_back(make(9, 64, 64, {64, 64, 64, 64}, {}));           // the stride over pixels
    cases.push_back(make(8, 128, 112, {20, 44, 13}, {}));             // ... with a stride the chunk count does not divide
    cases.push_back(make(4, 64, 64, {24, 100, 3, 5}, {1, 2, 4, 1}));
    return cases;
}

static std::vector<Case> builtin_requant() {
    std::vector<Case> cases;
    const int planes[][3] = {{1, 1, 1}, {1, 2, 2}, {3, 4, 12}, {2, 8, 8}};
    const std::vector<std::vector<int>> chans = {{16}, {3}, {16, 16}, {64, 64}, {1, 3}, {19, 33}, {100, 16, 1}, {33, 19, 3},
                                                 {16, 32, 48}, {1, 3, 16, 19, 33, 100, 1, 3}, {16, 16, 16, 16, 16, 16, 16, 16}};
    const std::vector<std::vector<int>> sizes = {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 2, 2, 2, 2, 2, 2, 2}, {1, 2, 1, 2, 2, 1, 2, 1},
                                                 {2, 1, 2, 1, 1, 2, 1, 2}};
    const std::vector<std::vector<int>> factors = {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 1, 4, 1, 2, 1, 4, 1}, {4, 2, 1, 4, 1, 2, 1, 4}};
    for (const auto& ch : chans)
        for (const auto& pl : planes)
            for (const auto& by : sizes)
                for (const auto& f : factors) {
                    bool ok = true;
                    for (size_t i = 0; i < ch.size(); ++i) ok = ok && pl[1] % f[i] == 0 && pl[2] % f[i] == 0;
                    if (ok) cases.push_back(make(pl[0], pl[1], pl[2], ch, f, by));
                }
    cases.push_back(make(3, 120, 120, {100, 100}, {1, 2}, {2, 1}));     // more chunks than the launch has lanes: the stride over pixels
    cases.push_back(make(9, 64, 64, {64, 64, 64, 64}, {}, {2, 1, 1, 2}));
    return cases;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    int maxsrc = 8;
    bool requant = false;
    for (int a = 1; a < argc; ++a) {
        if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
        if (strncmp(argv[a], "maxsrc=", 7) == 0) {
            maxsrc = atoi(argv[a] + 7);
            if (maxsrc != 2 && maxsrc != 8) {
                printf("maxsrc is 2 or 8\n");
                return 2;
            }
            continue;
        }
        Case c;
        if (!parse(argv[a], c)) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        requant = requant || c.requant;
        cases.push_back(c);
    }
    long total = 0;
    if (!cases.empty()) {
        for (const Case& c : cases) total += !c.requant && maxsrc == 2 ? run<2>(c, true) : run<8>(c, true);
        if (requant) printf("%s\n%s\n", check_requant().c_str(), check_guards().c_str());
        printf("ok, %ld loads checked\n", total);
        return 0;
    }
    long moving = 0;
    for (const Case& c : builtin_moving()) {
        if (c.nsrc <= 2) moving += run<2>(c, false);
        moving += run<8>(c, false);
    }
    for (const Case& c : builtin_requant()) total += run<8>(c, false);
    const std::string rounding = check_requant(), guards = check_guards();
    printf("ok, %ld loads checked (%ld moving, %ld re-quantising); %s; %s\n", moving + total, moving, total, rounding.c_str(), guards.c_str());
    return 0;
}
