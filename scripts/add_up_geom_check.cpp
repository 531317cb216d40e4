// Host check of the address arithmetic of the resident add with a nearest-upsampled operand (csrc/fq_add_up_geom.h; the pattern of
// avgpool_i16_geom_check.cpp): every lane of every launch loads inside both sources, every access is 16-byte aligned, the coarse
// pixel of an output pixel (h, w) is (h / up, w / up) at the same channels and image, the digit-wise walk (add_up_next) lands on
// the item the flat index names, and every output element is written exactly once.
//   c++ -O2 -std=c++17 -o add_up_geom_check scripts/add_up_geom_check.cpp
//   ./add_up_geom_check                      the built-in list: the GPU tests' shapes and the FPN model's launch shapes
//   ./add_up_geom_check N,H,W,C,up ...       these cases instead
// Every case is walked for all four operand widths (x and y int8 or int16) with both outputs.  One line per case:
// "case N,H,W,C,up: items n blocks b second-items m", then "ok, <loads> loads checked".  Exit status 1 at the first violation.
// The walk below is the kernel's own: same launch size, same lane -> item stepping, on a model of memory in which each byte is
// its own address; each output byte counts its writes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_add_up_geom.h"

using namespace fq;

struct Case { int N, H, W, C, up; };

static void fail(const char* what, const Case& c) {
    printf("%s: N %d, H %d, W %d, C %d, up %d\n", what, c.N, c.H, c.W, c.C, c.up);
    exit(1);
}

// a 16 * bytes wide access at item offset `item` of a tensor of `total` bytes: aligned pieces of 16 bytes inside it
static void access(size_t item, int bytes, size_t total, const char* what, const Case& c) {
    for (int piece = 0; piece < bytes; ++piece) {
        const size_t off = item * 16 * (size_t)bytes + 16 * (size_t)piece;
        if (off % 16 || off + 16 > total) fail(what, c);
    }
}

static long run(const Case& c, bool print) {
    if (c.N < 1 || c.H < 1 || c.W < 1 || c.C < 1 || add_up_log2(c.up) < 0 || c.H % c.up || c.W % c.up)
        fail("not a case the entry point launches", c);
    const int Cpad = (c.C + 15) / 16 * 16;
    const AddUpGeom g = add_up_geom(c.N, c.H, c.W, Cpad, c.up);
    if ((1 << g.lg) != c.up || g.Hc * c.up != c.H || g.Wc * c.up != c.W || g.CH * 16 != Cpad) fail("geometry", c);
    if (g.items != (size_t)c.N * c.H * c.W * g.CH) fail("item count", c);
    const unsigned blocks = add_up_blocks(g.items);
    if (blocks < 1 || blocks > (unsigned)kAddUpMaxBlocks) fail("launch size", c);
    const size_t threads = (size_t)blocks * kAddUpBlock;
    if (threads < g.items && blocks != (unsigned)kAddUpMaxBlocks) fail("fewer lanes than items below the cap", c);
    if (add_up_fine(g, g.step) != threads && threads < g.items) fail("the split of the stride", c);
    const size_t coarse_items = (size_t)c.N * g.Hc * g.Wc * g.CH;
    std::vector<unsigned char> written(g.items, 0);         // per item: the 16 / 32 output bytes of one item are one store group
    long loads = 0, second = 0;
    for (int xb = 1; xb <= 2; ++xb)
        for (int yb = 1; yb <= 2; ++yb) {
            std::fill(written.begin(), written.end(), 0);
            for (size_t t = 0; t < threads; ++t) {
                size_t i = t;
                if (i >= g.items) continue;
                AddUpItem it = add_up_first(g, i);
                for (int round = 0;; ++round) {
                    if (it.n < 0 || it.n >= c.N || it.h < 0 || it.h >= c.H || it.w < 0 || it.w >= c.W || it.k < 0 || it.k >= g.CH)
                        fail("item outside the output", c);
                    if (add_up_fine(g, it) != i) fail("the walk left the flat index", c);
                    const size_t cy = add_up_coarse(g, it);
                    if (cy != (((size_t)it.n * g.Hc + it.h / c.up) * g.Wc + it.w / c.up) * g.CH + it.k) fail("coarse pixel is not (h / up, w / up)", c);
                    if (cy >= coarse_items) fail("load outside the coarse source", c);
                    access(i, xb, (size_t)xb * 16 * g.items, "load outside x or unaligned", c);
                    access(cy, yb, (size_t)yb * 16 * coarse_items, "load outside y or unaligned", c);
                    access(i, 2, 32 * g.items, "wide store outside the output or unaligned", c);
                    access(i, 1, 16 * g.items, "narrow store outside the output or unaligned", c);
                    if (written[i]++) fail("output element written twice", c);
                    loads += xb + yb;
                    second += round == 1 && xb == 1 && yb == 1;
                    i += threads;
                    if (i >= g.items) break;
                    it = add_up_next(g, it);
                }
            }
            for (unsigned char v : written)
                if (v != 1) fail("output element not written", c);
        }
    if (print) printf("case %d,%d,%d,%d,%d: items %zu blocks %u second-items %ld\n", c.N, c.H, c.W, c.C, c.up, g.items, blocks, second);
    return loads;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        Case c;
        if (sscanf(argv[a], "%d,%d,%d,%d,%d", &c.N, &c.H, &c.W, &c.C, &c.up) != 5) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(c);
    }
    if (cases.empty()) {
        const int planes[][2] = {{2, 2}, {4, 4}, {4, 12}, {8, 8}};
        const int chans[] = {1, 16, 19, 100};
        for (int up : {2, 4})
            for (int N : {1, 3})
                for (const auto& pl : planes)
                    for (int C : chans)
                        if (pl[0] % up == 0 && pl[1] % up == 0) cases.push_back(Case{N, pl[0], pl[1], C, up});
        cases.push_back(Case{1, 592, 592, 48, 2});           // 1 051 392 items: the smallest square plane at 48 channels past 4096 x 256 lanes
        cases.push_back(Case{1, 592, 592, 48, 4});
        cases.push_back(Case{2, 4, 4, 256, 2});              // ResNet50FPN at 64 x 64, batch 2: P4 and P3
        cases.push_back(Case{2, 8, 8, 256, 2});
        cases.push_back(Case{256, 14, 14, 256, 2});           // ... at 224 x 224: P4 and P3 (the cost script: 256 images)
        cases.push_back(Case{256, 28, 28, 256, 2});
    }
    long total = 0;
    for (const Case& c : cases) total += run(c, true);
    printf("ok, %ld loads checked\n", total);
    return 0;
}
