// Host check of the address arithmetic of the windowed average pool over an int16 sum (csrc/fq_avgpool_i16_geom.h, the twin of
// avgpool_geom_check.cpp): every lane of every launch loads inside the source (16 bytes, aligned), the taps of an output are
// exactly window ∩ image, each once, the divisor is the rule's, the channel mask keeps the real channels only, and every output
// byte is written exactly once and inside the output.
//   c++ -O2 -std=c++17 -o avgpool_i16_geom_check scripts/avgpool_i16_geom_check.cpp
//   ./avgpool_i16_geom_check                                  the built-in shape list
//   ./avgpool_i16_geom_check N,H,W,C,kh,kw,sh,sw,ph,pw ...    these cases instead; tests pass the GPU tests' list
// Every case is walked with and without count_include_pad.  One line per case: "case ...: P p Q q items n blocks b", then
// "ok, <loads> loads checked".  Exit status 1 at the first violation.
// The walk below is the kernel's own: same launch size, same lane -> item stepping by the grid size, the same window cut and the
// same offset stepping along a window row, on a model of memory in which each byte is its own address: a load is 16 byte
// addresses of the source, a store 8 byte addresses of the output, and each output byte counts its writes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_avgpool_i16_geom.h"

using namespace fq;

struct Case { int N, H, W, C, kh, kw, sh, sw, ph, pw; };

static void fail(const char* what, const Case& c, int cip) {
    printf("%s: N %d, H %d, W %d, C %d, kernel %dx%d, stride %d,%d, padding %d,%d, count_include_pad %d\n", what, c.N, c.H, c.W, c.C,
           c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, cip);
    exit(1);
}

static long run(const Case& c, int cip, bool print) {
    if (c.N < 1 || c.H < 1 || c.W < 1 || c.C < 1 || c.kh < 1 || c.kw < 1 || c.sh < 1 || c.sw < 1 || c.ph < 0 || c.pw < 0 ||
        2 * c.ph > c.kh || 2 * c.pw > c.kw || c.kh * c.kw > kAvgMaxTaps)
        fail("not a case the entry point launches", c, cip);
    const int Cpad = (c.C + 15) / 16 * 16;
    const AvgGeom g = avg16_geom(c.N, c.H, c.W, c.C, Cpad, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, cip);
    if (g.P < 1 || g.Q < 1) fail("empty output", c, cip);
    if (g.P != (c.H + 2 * c.ph - c.kh) / c.sh + 1 || g.Q != (c.W + 2 * c.pw - c.kw) / c.sw + 1) fail("output size is not floor mode's", c, cip);
    const long x_bytes = 2L * c.N * c.H * c.W * Cpad, y_bytes = (long)c.N * g.P * g.Q * Cpad;
    if (x_bytes >= 0x7fffffffL || y_bytes >= 0x7fffffffL) fail("tensor too large for the entry point", c, cip);
    if (g.CH * kAvg16Lane != Cpad || (long)g.nchunks * kAvg16Lane != y_bytes) fail("the items do not tile the output", c, cip);
    const long blocks = avg_blocks(g);
    if (blocks < 1 || blocks > kAvgMaxBlocks) fail("launch size", c, cip);
    if (print && cip)
        printf("case %d,%d,%d,%d,%d,%d,%d,%d,%d,%d: P %d Q %d items %u blocks %ld\n", c.N, c.H, c.W, c.C, c.kh, c.kw, c.sh, c.sw, c.ph,
               c.pw, g.P, g.Q, g.nchunks, blocks);

    const unsigned threads = (unsigned)blocks * kAvgBlock;
    if ((unsigned long)g.nchunks + threads > 0xffffffffUL) fail("the 32-bit item index wraps in `i += stride`", c, cip);
    std::vector<unsigned char> written((size_t)y_bytes, 0);
    const unsigned step = avg16_tap_step(g);
    long loads = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        for (unsigned i = gid; i < g.nchunks; i += threads) {
            const AvgChunk ch = avg_chunk(g, i);
            if (ch.n < 0 || ch.n >= c.N || ch.p < 0 || ch.p >= g.P || ch.q < 0 || ch.q >= g.Q || ch.k < 0 || ch.k >= g.CH)
                fail("item index outside the output", c, cip);
            if ((((long)ch.n * g.P + ch.p) * g.Q + ch.q) * g.CH + ch.k != (long)i) fail("item is not where it is stored", c, cip);
            const AvgWindow w = avg_window(g, ch.p, ch.q);
            // the kernel's loads
            std::set<std::pair<int, int>> got;
            for (int ih = w.h0; ih < w.h1; ++ih) {
                unsigned off = avg16_tap_offset(g, ch.n, ih, w.w0, ch.k);
                for (int iw = w.w0; iw < w.w1; ++iw, off += step) {
                    const long o = (long)off;
                    if (o % 16 || o < 0 || o + 16 > x_bytes) fail("16-byte load outside the source or unaligned", c, cip);
                    if (ih < 0 || ih >= c.H || iw < 0 || iw >= c.W) fail("tap outside the image", c, cip);
                    // the first of its eight int16: channel 8 k of pixel (n, ih, iw)
                    if (o != 2L * ((((long)ch.n * c.H + ih) * c.W + iw) * Cpad + (long)kAvg16Lane * ch.k)) fail("load is not the tap's address", c, cip);
                    if (!got.insert(std::make_pair(ih, iw)).second) fail("tap loaded twice", c, cip);
                    ++loads;
                }
            }
            // the rule: window ∩ image
            std::set<std::pair<int, int>> want;
            for (int a = 0; a < c.kh; ++a)
                for (int b = 0; b < c.kw; ++b) {
                    const int ih = ch.p * c.sh - c.ph + a, iw = ch.q * c.sw - c.pw + b;
                    if (ih >= 0 && ih < c.H && iw >= 0 && iw < c.W) want.insert(std::make_pair(ih, iw));
                }
            if (want.empty()) fail("empty window", c, cip);
            if (got != want) fail("the taps are not window ∩ image", c, cip);
            int rows = 0, cols = 0;
            for (int a = 0; a < c.kh; ++a) rows += ch.p * c.sh - c.ph + a >= 0 && ch.p * c.sh - c.ph + a < c.H;
            for (int b = 0; b < c.kw; ++b) cols += ch.q * c.sw - c.pw + b >= 0 && ch.q * c.sw - c.pw + b < c.W;
            if (avg_divisor(g, w) != (cip ? c.kh * c.kw : rows * cols) || avg_divisor(g, w) < 1 || avg_divisor(g, w) > kAvgMaxTaps)
                fail("divisor", c, cip);
            for (int t = 0; t < 2; ++t) {
                const unsigned m = avg16_dword_mask(g, ch.k, t);
                for (int j = 0; j < 4; ++j)
                    if (((m >> (8 * j)) & 0xffu) != (kAvg16Lane * ch.k + 4 * t + j < c.C ? 0xffu : 0u)) fail("channel mask", c, cip);
            }
            // the 8-byte store: aligned, inside the output, at the item's own channels, every byte for the first time
            const size_t so = avg16_store_offset(i);
            if (so % 8 || (long)so + kAvg16Lane > y_bytes) fail("store outside the output or unaligned", c, cip);
            if ((long)so != (((long)ch.n * g.P + ch.p) * g.Q + ch.q) * Cpad + (long)kAvg16Lane * ch.k) fail("store is not the item's address", c, cip);
            for (int j = 0; j < kAvg16Lane; ++j)
                if (written[so + j]++) fail("output byte written twice", c, cip);
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output byte not written", c, cip);
    return loads;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        Case c;
        if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", &c.N, &c.H, &c.W, &c.C, &c.kh, &c.kw, &c.sh, &c.sw, &c.ph, &c.pw) != 10) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(c);
    }
    if (cases.empty()) {
        const int planes[][3] = {{1, 1, 1}, {1, 2, 2}, {2, 3, 5}, {3, 5, 7}, {1, 9, 11}};
        const int chans[] = {1, 8, 9, 16, 19, 100};
        const int wins[][6] = {{3, 3, 1, 1, 1, 1}, {3, 3, 1, 1, 0, 0}, {2, 2, 2, 2, 0, 0}, {2, 2, 2, 2, 1, 1}, {3, 3, 2, 2, 1, 1}, {3, 3, 2, 2, 0, 0},
                               {5, 5, 1, 1, 2, 2}, {5, 5, 3, 3, 2, 2}, {2, 3, 1, 2, 1, 1}, {7, 7, 1, 1, 3, 3}, {8, 8, 8, 8, 4, 4}, {1, 1, 1, 1, 0, 0},
                               {1, 64, 1, 3, 0, 32}, {4, 1, 5, 1, 2, 0}};
        for (const auto& pl : planes)
            for (int C : chans)
                for (const auto& k : wins) {
                    if (pl[1] + 2 * k[4] < k[0] || pl[2] + 2 * k[5] < k[1]) continue;
                    cases.push_back(Case{pl[0], pl[1], pl[2], C, k[0], k[1], k[2], k[3], k[4], k[5]});
                }
        cases.push_back(Case{2, 129, 129, 128, 3, 3, 1, 1, 1, 1});     // more items than the launch has lanes: the stride over items
        cases.push_back(Case{8, 56, 56, 256, 2, 2, 2, 2, 0, 0});       // the ResNet-D shortcut in front of stage 2
    }
    long total = 0;
    for (const Case& c : cases)
        for (int cip = 0; cip < 2; ++cip) total += run(c, cip, argc > 1);
    printf("ok, %ld loads checked\n", total);
    return 0;
}
