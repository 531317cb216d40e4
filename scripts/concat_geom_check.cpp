// Host check of the concat / nearest-upsampling kernel's address arithmetic (csrc/fq_concat_i8_geom.h): every lane of every
// launch loads inside its source (aligned, a dword or 16 bytes), assembles exactly the bytes the index rule asks for, and every
// output chunk is written exactly once.
//   c++ -O2 -std=c++17 -o concat_geom_check scripts/concat_geom_check.cpp
//   ./concat_geom_check                         the built-in shape list
//   ./concat_geom_check N,H,W,C0,C1,up0,up1 ...  these cases instead (C1 == 0: one source); tests pass the GPU tests' list
//   ./concat_geom_check window=P <cases>         a size-limit row (10^8 chunks): only the first and the last P pixels of the
//                                                output are walked, by the lanes and in the order the kernel visits them; no
//                                                tensor reaches 2^31 bytes, so there is no boundary between
// One line per case: "case N,H,W,C0,C1,up0,up1: aligned16 A dword D byte B straddle S" (chunks of one pixel by
// cat_chunk_class), then "ok, <loads> loads checked".  Exit status 1 at the first violation.
// The walk below is the kernel's own: same launch size, same lane -> (chunk, first pixel, stride), the same predicates in
// front of every load; the bytes are carried through the same shift-and-mask steps on a model of memory whose every byte is
// its own address, so that a wrong byte is seen as well as a wrong address.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_concat_i8_geom.h"

using namespace fq;

struct Case { int N, H, W, C[2], up[2]; };

static void fail(const char* what, const Case& c) {
    printf("%s: N %d, H %d, W %d, C0 %d, C1 %d, up0 %d, up1 %d\n", what, c.N, c.H, c.W, c.C[0], c.C[1], c.up[0], c.up[1]);
    exit(1);
}

// v_alignbyte_b32: ({hi, lo} >> 8 * sh) & 0xffffffff on "addresses" instead of bytes: byte j of the result is byte sh + j of the
// pair; -1 marks a byte of a dword that was not loaded
static void alignbyte(const long (&hi)[4], const long (&lo)[4], int sh, long (&out)[4]) {
    for (int j = 0; j < 4; ++j) out[j] = sh + j < 4 ? lo[sh + j] : hi[sh + j - 4];
}

static unsigned long g_window = 0;          // window=P: pixels [P, npix - P) are skipped

static long run(const Case& c, bool print) {
    CatGeom g;
    g.nsrc = c.C[1] > 0 ? 2 : 1;
    long src_bytes[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        g.s[i].C = i < g.nsrc ? c.C[i] : 0;
        g.s[i].Cpad = i < g.nsrc ? (c.C[i] + 15) / 16 * 16 : 16;
        g.s[i].lu = c.up[i] == 4 ? 2 : (c.up[i] == 2 ? 1 : 0);
        if (i < g.nsrc) {
            if (c.H % c.up[i] || c.W % c.up[i]) fail("plane is no multiple of the factor", c);
            src_bytes[i] = (long)c.N * (c.H / c.up[i]) * (c.W / c.up[i]) * g.s[i].Cpad;
        }
    }
    g.N = c.N; g.H = c.H; g.W = c.W;
    const int sum = c.C[0] + (g.nsrc == 2 ? c.C[1] : 0);
    g.Cpad_out = (sum + 15) / 16 * 16;
    g.CH = g.Cpad_out / 16;
    g.npix = (unsigned)((long)c.N * c.H * c.W);
    const bool general = g.nsrc == 2 && c.C[0] % 16 != 0;
    int cls[4] = {0, 0, 0, 0};
    for (int k = 0; k < g.CH; ++k) ++cls[cat_chunk_class(g, k)];
    if (!general && (cls[kCatDword] || cls[kCatByte] || cls[kCatStraddle])) fail("an aligned launch holds a chunk that is not one 16-byte load", c);
    if (print)
        printf("case %d,%d,%d,%d,%d,%d,%d: aligned16 %d dword %d byte %d straddle %d\n", c.N, c.H, c.W, c.C[0], c.C[1], c.up[0], c.up[1],
               cls[0], cls[1], cls[2], cls[3]);

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
        CatPart part[2] = {cat_part(g, k, 0), cat_part(g, k, 1)};
        if (!general) {                                   // the kernel picks the one owner and masks the tail only
            const int i = part[1].use ? 1 : 0;
            if (!part[i].use || !part[i].whole16 || part[1 - i].use) fail("aligned launch: the chunk is not 16 bytes of one source", c);
        }
        for (; pix < g.npix; pix += stride) {
            if (windowed && pix >= g_window && pix < g.npix - g_window) {      // jump to this lane's first pixel of the last window
                const unsigned long steps = ((unsigned long)(g.npix - g_window) - pix + stride - 1) / stride;
                const unsigned long next = pix + steps * stride;
                if (next >= g.npix) break;
                pix = (unsigned)(next - stride);
                continue;
            }
            // the bytes the kernel assembles, as (source, address) pairs; got[j] = -1: zero
            long got[16];
            int got_src[16];
            for (int j = 0; j < 16; ++j) { got[j] = -1; got_src[j] = -1; }
            for (int i = 0; i < g.nsrc; ++i) {
                const CatPart& p = part[i];
                if (!p.use) continue;
                const unsigned sp = cat_src_pix(g, i, pix);
                const long row = (long)sp * g.s[i].Cpad;
                const bool one16 = general ? (i == 0 && p.whole16 && !part[1].use) : true;
                long bytes[16];
                if (one16) {
                    const long o = row + p.s;
                    if (o < 0 || o % 16 || o + 16 > src_bytes[i]) fail("16-byte load outside its source or unaligned", c);
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
                    const unsigned m = cat_dword_mask(general && !one16 ? p.lo : 0, p.hi, t);
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
            const unsigned w = pix % g.W, h = (pix / g.W) % g.H, n = pix / g.W / g.H;
            for (int j = 0; j < 16; ++j) {
                const int ch = 16 * k + j;
                int i = -1, cc = 0;
                if (ch < c.C[0]) { i = 0; cc = ch; }
                else if (g.nsrc == 2 && ch < c.C[0] + c.C[1]) { i = 1; cc = ch - c.C[0]; }
                long want = -1;
                if (i >= 0) {
                    const int u = c.up[i];
                    want = (((long)n * (c.H / u) + h / u) * (c.W / u) + w / u) * g.s[i].Cpad + cc;
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

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
        Case c;
        if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &c.N, &c.H, &c.W, &c.C[0], &c.C[1], &c.up[0], &c.up[1]) != 7) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(c);
    }
    if (cases.empty()) {
        const int chans[][2] = {{16, 16}, {64, 64}, {20, 44}, {3, 5}, {17, 30}, {13, 3}, {1, 1}, {24, 8}, {5, 7}, {15, 1}, {1, 15},
                                {31, 33}, {4, 12}, {100, 28}, {3, 0}, {16, 0}, {40, 0}};
        const int planes[][3] = {{1, 1, 1}, {2, 3, 5}, {1, 4, 4}, {3, 7, 9}, {2, 8, 12}};
        for (const auto& ch : chans)
            for (const auto& pl : planes)
                for (int u0 : {1, 2, 4})
                    for (int u1 : {1, 2, 4}) {
                        if (pl[1] % u0 || pl[2] % u0 || pl[1] % u1 || pl[2] % u1 || (ch[1] == 0 && u1 != 1)) continue;
                        cases.push_back(Case{pl[0], pl[1], pl[2], {ch[0], ch[1]}, {u0, u1}});
                    }
        cases.push_back(Case{64, 56, 56, {64, 64}, {1, 1}});          // more chunks than the launch has lanes: the stride over pixels
        cases.push_back(Case{16, 52, 52, {24, 100}, {1, 2}});
    }
    long total = 0;
    for (const Case& c : cases) total += run(c, argc > 1);
    printf("ok, %ld loads checked\n", total);
    return 0;
}
