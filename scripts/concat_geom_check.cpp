// Host check of the concat / nearest-upsampling kernel's address arithmetic (csrc/fq_concat_i8_geom.h), for both instantiations
// of the kernel (MAXSRC = 2: fq_concat_i8_nhwc, MAXSRC = 8: fq_concat_n_i8_nhwc): every lane of every launch loads inside its
// source (aligned, a dword or 16 bytes), assembles exactly the bytes the index rule asks for, every output chunk is written
// exactly once, and an aligned launch is made of 16-byte loads only.
//   c++ -O2 -std=c++17 -o concat_geom_check scripts/concat_geom_check.cpp
//   ./concat_geom_check                                     the built-in shape list: cases of one or two sources at both limits,
//                                                           the rest at 8
//   ./concat_geom_check N,H,W/C0,C1,.../up0,up1,... ...      these cases instead; tests pass the GPU tests' list
//   ./concat_geom_check maxsrc=2|8 <cases>                  the instantiation whose geometry is walked (default 8); a case with
//                                                           more sources is an error
//   ./concat_geom_check window=P <cases>                    a size-limit row (10^8 chunks): only the first and the last P pixels
//                                                           of the output are walked, by the lanes and in the order the kernel
//                                                           visits them; no tensor reaches 2^31 bytes, so there is no boundary between
// One line per case: "case N,H,W/C.../up...: aligned16 A dword D byte B straddle S" (chunks of one pixel by cat_chunk_class),
// then "ok, <loads> loads checked".  Exit status 1 at the first violation.
// The walk below is the kernel's own: same launch size, same lane -> (chunk, first pixel, stride), the same predicates in
// front of every load; the bytes are carried through the same shift-and-mask steps on a model of memory whose every byte is
// its own address, so that a wrong byte is seen as well as a wrong address.  (The per-source ReLU acts on values, not on
// addresses: it is applied to each masked part in front of the or and has no place in this model.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_concat_i8_geom.h"

using namespace fq;

constexpr int kMaxSrc = 8;
struct Case { int N, H, W, nsrc, C[kMaxSrc], up[kMaxSrc]; std::string text; };

static void fail(const char* what, const Case& c) {
    printf("%s: %s\n", what, c.text.c_str());
    exit(1);
}

static std::string text_of(const Case& c) {
    std::string s = std::to_string(c.N) + "," + std::to_string(c.H) + "," + std::to_string(c.W) + "/";
    for (int i = 0; i < c.nsrc; ++i) s += (i ? "," : "") + std::to_string(c.C[i]);
    s += "/";
    for (int i = 0; i < c.nsrc; ++i) s += (i ? "," : "") + std::to_string(c.up[i]);
    return s;
}

// v_alignbyte_b32: ({hi, lo} >> 8 * sh) & 0xffffffff on "addresses" instead of bytes: byte j of the result is byte sh + j of the
// pair; -2 marks a byte of a dword that was not loaded
static void alignbyte(const long (&hi)[4], const long (&lo)[4], int sh, long (&out)[4]) {
    for (int j = 0; j < 4; ++j) out[j] = sh + j < 4 ? lo[sh + j] : hi[sh + j - 4];
}

static unsigned long g_window = 0;          // window=P: pixels [P, npix - P) are skipped

template <int MAXSRC>
static long run(const Case& c, bool print) {
    if (c.nsrc > MAXSRC) fail("more sources than maxsrc", c);
    CatGeom<MAXSRC> g;
    g.nsrc = c.nsrc;
    long src_bytes[MAXSRC];
    int base = 0;
    for (int i = 0; i < MAXSRC; ++i) {
        const bool have = i < c.nsrc;
        g.s[i].C = have ? c.C[i] : 0;
        g.s[i].Cpad = have ? (c.C[i] + 15) / 16 * 16 : 16;
        g.s[i].lu = have ? (c.up[i] == 4 ? 2 : (c.up[i] == 2 ? 1 : 0)) : 0;
        g.s[i].base = base;
        base += g.s[i].C;
        src_bytes[i] = 0;
        if (have) {
            if (c.C[i] < 1 || (c.up[i] != 1 && c.up[i] != 2 && c.up[i] != 4)) fail("bad channel count or factor", c);
            if (c.H % c.up[i] || c.W % c.up[i]) fail("plane is no multiple of the factor", c);
            src_bytes[i] = (long)c.N * (c.H / c.up[i]) * (c.W / c.up[i]) * g.s[i].Cpad;
        }
    }
    const int sum = base;
    g.N = c.N; g.H = c.H; g.W = c.W;
    g.Cpad_out = (sum + 15) / 16 * 16;
    g.CH = g.Cpad_out / 16;
    g.npix = (unsigned)((long)c.N * c.H * c.W);
    const bool general = !cat_aligned(g);
    int cls[4] = {0, 0, 0, 0};
    for (int k = 0; k < g.CH; ++k) ++cls[cat_chunk_class(g, k)];
    if (!general && (cls[kCatDword] || cls[kCatByte] || cls[kCatStraddle])) fail("an aligned launch holds a chunk that is not one 16-byte load", c);
    if (print) printf("case %s: aligned16 %d dword %d byte %d straddle %d\n", c.text.c_str(), cls[0], cls[1], cls[2], cls[3]);

    const unsigned threads = (unsigned)cat_blocks(g) * kCatBlock, stride = threads / g.CH;
    // the kernel's pixel index, lane number and `pix += stride` are 32 bits wide
    if ((unsigned long)g.npix + stride > 0xffffffffUL || (unsigned long)g.npix * g.CH > 0xffffffffUL) fail("32-bit pixel arithmetic wraps", c);
    const bool windowed = g_window && (unsigned long)g.npix > 2 * g_window;
    const unsigned long walked = windowed ? 2 * g_window : g.npix;
    auto slot = [&](unsigned pix) { return !windowed || pix < g_window ? (size_t)pix : (size_t)(g_window + (pix - (g.npix - g_window))); };
    std::vector<unsigned char> written((size_t)walked * g.CH, 0);
    long loads = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int k = gid % g.CH;
        unsigned pix = gid / g.CH;
        if (pix >= stride) continue;
        CatPart part[MAXSRC];
        int owners = 0, whole = 0;
        for (int i = 0; i < MAXSRC; ++i) {
            part[i] = cat_part(g, k, i);
            owners += part[i].use;
            whole |= part[i].use & part[i].whole16;
        }
        const bool one16 = owners == 1 && whole;            // the kernel's test in front of cat_loop16
        if (!general && !one16) fail("aligned launch: the chunk is not 16 bytes of one source", c);
        for (int i = 0; i < MAXSRC; ++i)
            if (one16 != cat_one16(g, k, i) && part[i].use) fail("cat_one16 disagrees with the kernel's test", c);
        for (; pix < g.npix; pix += stride) {
            if (windowed && pix >= g_window && pix < g.npix - g_window) {      // jump to this lane's first pixel of the last window
                const unsigned long steps = ((unsigned long)(g.npix - g_window) - pix + stride - 1) / stride;
                const unsigned long next = pix + steps * stride;
                if (next >= g.npix) break;
                pix = (unsigned)(next - stride);
                continue;
            }
            const unsigned w = pix % g.W, h = (pix / g.W) % g.H, n = pix / g.W / g.H;
            // the bytes the kernel assembles, as (source, address) pairs; got[j] = -1: zero
            long got[16];
            int got_src[16];
            for (int j = 0; j < 16; ++j) { got[j] = -1; got_src[j] = -1; }
            for (int i = 0; i < MAXSRC; ++i) {
                const CatPart& p = part[i];
                if (!(i < g.nsrc) || !p.use) continue;
                if (!one16 && !p.ld) fail("a used part loads nothing", c);
                const unsigned sp = cat_src_pix(g, g.s[i].lu, n, h, w);
                if (g.s[i].lu == 0 && sp != pix) fail("source pixel of a source that is not upsampled", c);
                const long row = (long)sp * g.s[i].Cpad;
                long bytes[16];
                if (one16) {
                    const long o = row + p.s;
                    if (o < 0 || o % 16 || o + 16 > src_bytes[i]) fail("16-byte load outside its source or unaligned", c);
                    if (p.s < 0 || p.s + 16 > g.s[i].Cpad) fail("16-byte load outside its pixel row", c);
                    ++loads;
                    for (int j = 0; j < 16; ++j) bytes[j] = o + j;
                } else {
                    long d[5][4];
                    for (int t = 0; t < 5; ++t) {
                        for (int j = 0; j < 4; ++j) d[t][j] = -2;                   // not loaded: zero in the kernel
                        if (!(p.ld & (1u << t))) continue;
                        const long o = row + p.a + 4 * t;
                        if (o < 0 || o % 4 || o + 4 > src_bytes[i]) fail("dword load outside its source or unaligned", c);
                        if (p.a + 4 * t < 0 || p.a + 4 * t + 4 > g.s[i].Cpad) fail("dword load outside its pixel row", c);
                        ++loads;
                        for (int j = 0; j < 4; ++j) d[t][j] = o + j;
                    }
                    for (int t = 0; t < 4; ++t) {
                        long o4[4];
                        alignbyte(d[t + 1], d[t], p.sh, o4);
                        for (int j = 0; j < 4; ++j) bytes[4 * t + j] = o4[j];
                    }
                }
                for (int t = 0; t < 4; ++t) {
                    const unsigned m = cat_dword_mask(one16 ? 0 : p.lo, p.hi, t);
                    for (int j = 0; j < 4; ++j) {
                        if (!((m >> (8 * j)) & 0xffu)) continue;
                        if (((m >> (8 * j)) & 0xffu) != 0xffu) fail("partial byte mask", c);
                        if (got[4 * t + j] != -1) fail("two sources write one output byte", c);
                        if (bytes[4 * t + j] < 0) fail("a wanted byte comes from a dword that was not loaded", c);
                        got[4 * t + j] = bytes[4 * t + j];
                        got_src[4 * t + j] = i;
                    }
                }
            }
            // the index rule
            for (int j = 0; j < 16; ++j) {
                const int ch = 16 * k + j;
                int i = -1;
                for (int q = 0; q < c.nsrc; ++q)
                    if (ch >= g.s[q].base && ch < g.s[q].base + c.C[q]) i = q;
                long want = -1;
                if (i >= 0) {
                    const int u = c.up[i];
                    want = (((long)n * (c.H / u) + h / u) * (c.W / u) + w / u) * g.s[i].Cpad + (ch - g.s[i].base);
                }
                if (got[j] != want || got_src[j] != i) fail("output byte is not the byte the index rule names", c);
            }
            const size_t chunk = (size_t)pix * g.CH + k;
            if ((chunk + 1) * 16 > (size_t)g.npix * g.Cpad_out) fail("store outside the output", c);
            if (written[slot(pix) * g.CH + k]++) fail("output chunk written twice", c);
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output chunk not written", c);
    return loads;
}

static bool parse_list(const char* s, int* out, int& n) {
    n = 0;
    while (*s) {
        char* end;
        const long v = strtol(s, &end, 10);
        if (end == s || n >= kMaxSrc) return false;
        out[n++] = (int)v;
        s = *end == ',' ? end + 1 : end;
        if (*end && *end != ',') return false;
    }
    return n > 0;
}

static bool parse(const char* arg, Case& c) {
    std::string a(arg);
    const size_t p1 = a.find('/'), p2 = a.find('/', p1 == std::string::npos ? 0 : p1 + 1);
    if (p1 == std::string::npos || p2 == std::string::npos) return false;
    if (sscanf(a.substr(0, p1).c_str(), "%d,%d,%d", &c.N, &c.H, &c.W) != 3) return false;
    int nc = 0, nu = 0;
    if (!parse_list(a.substr(p1 + 1, p2 - p1 - 1).c_str(), c.C, nc) || !parse_list(a.substr(p2 + 1).c_str(), c.up, nu) || nc != nu)
        return false;
    c.nsrc = nc;
    c.text = text_of(c);
    return c.N > 0 && c.H > 0 && c.W > 0;
}

static Case make(int N, int H, int W, std::vector<int> C, std::vector<int> up) {
    Case c;
    c.N = N; c.H = H; c.W = W; c.nsrc = (int)C.size();
    for (int i = 0; i < c.nsrc; ++i) { c.C[i] = C[i]; c.up[i] = i < (int)up.size() ? up[i] : 1; }
    c.text = text_of(c);
    return c;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    int maxsrc = 8;
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
        cases.push_back(c);
    }
    long total = 0;
    if (!cases.empty()) {
        for (const Case& c : cases) total += maxsrc == 2 ? run<2>(c, true) : run<8>(c, true);
        printf("ok, %ld loads checked\n", total);
        return 0;
    }
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
    for (const Case& c : cases) {
        if (c.nsrc <= 2) total += run<2>(c, false);
        total += run<8>(c, false);
    }
    printf("ok, %ld loads checked\n", total);
    return 0;
}
