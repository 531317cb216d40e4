// Host check of the address arithmetic and the integer rule of the resident int8 bilinear upsampling
// (csrc/fq_upsample_bilinear_i8_geom.h; the pattern of add_up_geom_check.cpp): every lane of every launch loads inside the source,
// every access is 16-byte aligned, every output element is written exactly once, the digit-wise walk (upb_next) lands on the item
// the flat index names, the taps and weights a lane uses for output (up h + dy, up w + dx) are the closed form
//   t = max(2 o + 1 - up, 0), i0 = t div D, l1 = t mod D, l0 = D - l1, i1 = min(i0 + 1, H - 1)
// and upb_requant equals S 2^e rounded half to even (computed here in double) and clamped, for every S in [-8192, 8192], every
// shift in [-8, 8], both factors, with and without the ReLU.
//   c++ -O2 -std=c++17 -o upsample_bilinear_geom_check scripts/upsample_bilinear_geom_check.cpp
//   ./upsample_bilinear_geom_check                      the built-in list: the GPU tests' shapes and the U-Net's launch shapes
//   ./upsample_bilinear_geom_check N,H,W,C,up ...       these cases instead
// One line per case: "case N,H,W,C,up: items n blocks b second-items m", then "ok, <loads> loads checked".  Exit status 1 at the
// first violation.  The walk is the kernel's own: same launch size, same lane -> item stepping; each output chunk counts its writes.
// A plain program with its own main: -fsanitize=address,undefined applies as it stands.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_upsample_bilinear_i8_geom.h"

using namespace fq;

struct Case { int N, H, W, C, up; };

static void fail(const char* what, const Case& c) {
    printf("%s: N %d, H %d, W %d, C %d, up %d\n", what, c.N, c.H, c.W, c.C, c.up);
    exit(1);
}

// the closed form along one axis of `size` source elements: output o -> (i0, i1, l0, l1)
static void closed_form(int o, int up, int size, int* i0, int* i1, int* l0, int* l1) {
    const int D = 2 * up;
    int t = 2 * o + 1 - up;
    if (t < 0) t = 0;
    *i0 = t / D;
    *l1 = t % D;
    *l0 = D - *l1;
    *i1 = *i0 + 1 < size ? *i0 + 1 : size - 1;
}

// the lane's taps against the closed form: the same weighted multiset of source indices (at the borders two taps coincide)
static bool same_taps(int a0, int a1, int wa0, int wa1, int b0, int b1, int wb0, int wb1, int size) {
    std::vector<int> wa(size, 0), wb(size, 0);
    wa[a0] += wa0; wa[a1] += wa1;
    wb[b0] += wb0; wb[b1] += wb1;
    return wa == wb;
}

static long run(const Case& c, bool print) {
    if (c.N < 1 || c.H < 1 || c.W < 1 || c.C < 1 || upb_log2(c.up) < 0) fail("not a case the entry point launches", c);
    const int Cpad = (c.C + 15) / 16 * 16;
    if (upb_args(c.N, c.H, c.W, c.C, Cpad, c.up, 0) != 0) fail("refused by upb_args", c);
    const UpbGeom g = upb_geom(c.N, c.H, c.W, c.C, Cpad, c.up);
    if (g.CH * 16 != Cpad || g.Ho != c.up * c.H || g.Wo != c.up * c.W) fail("geometry", c);
    if ((size_t)g.items != (size_t)c.N * c.H * c.W * g.CH) fail("item count", c);
    const unsigned blocks = upb_blocks(g.items);
    if (blocks < 1 || blocks > (unsigned)kUpbMaxBlocks) fail("launch size", c);
    const size_t threads = (size_t)blocks * kUpbBlock;
    if (threads < g.items && blocks != (unsigned)kUpbMaxBlocks) fail("fewer lanes than items below the cap", c);
    const size_t src_bytes = (size_t)c.N * c.H * c.W * Cpad, dst_bytes = src_bytes * c.up * c.up;
    std::vector<unsigned char> written(dst_bytes / 16, 0);
    long loads = 0, second = 0;
    for (size_t t = 0; t < threads; ++t) {
        size_t i = t;
        if (i >= g.items) continue;
        UpbItem it = upb_first(g, (unsigned)i);
        for (int round = 0;; ++round) {
            if (it.n < 0 || it.n >= c.N || it.h < 0 || it.h >= c.H || it.w < 0 || it.w >= c.W || it.k < 0 || it.k >= g.CH)
                fail("item outside the source", c);
            if (upb_src_offset(g, it.n, it.h, it.w, it.k) != i * 16) fail("the walk left the flat index", c);
            const UpbNbr nb = upb_nbr(g, it);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    if (nb.row[a] < 0 || nb.row[a] >= c.H || nb.col[b] < 0 || nb.col[b] >= c.W) fail("tap outside the plane", c);
                    const size_t off = upb_src_offset(g, it.n, nb.row[a], nb.col[b], it.k);
                    if (off % 16 || off + 16 > src_bytes) fail("load outside x or unaligned", c);
                    ++loads;
                }
            for (int dy = 0; dy < c.up; ++dy)
                for (int dx = 0; dx < c.up; ++dx) {
                    const UpbTap ty = upb_tap(c.up, dy), tx = upb_tap(c.up, dx);
                    if (ty.first < 0 || ty.first > 1 || tx.first < 0 || tx.first > 1) fail("tap index", c);
                    if (ty.l0 + ty.l1 != 2 * c.up || tx.l0 + tx.l1 != 2 * c.up || ty.l0 < 1 || ty.l1 < 1 || tx.l0 < 1 || tx.l1 < 1)
                        fail("weights", c);
                    int i0, i1, l0, l1;
                    closed_form(c.up * it.h + dy, c.up, c.H, &i0, &i1, &l0, &l1);
                    if (!same_taps(nb.row[ty.first], nb.row[ty.first + 1], ty.l0, ty.l1, i0, i1, l0, l1, c.H))
                        fail("row taps are not the closed form", c);
                    closed_form(c.up * it.w + dx, c.up, c.W, &i0, &i1, &l0, &l1);
                    if (!same_taps(nb.col[tx.first], nb.col[tx.first + 1], tx.l0, tx.l1, i0, i1, l0, l1, c.W))
                        fail("column taps are not the closed form", c);
                    const size_t off = upb_dst_offset(g, it, dy, dx);
                    if (off % 16 || off + 16 > dst_bytes) fail("store outside y or unaligned", c);
                    const size_t want = ((((size_t)it.n * g.Ho + (size_t)(c.up * it.h + dy)) * g.Wo + (size_t)(c.up * it.w + dx)) * Cpad) + 16 * (size_t)it.k;
                    if (off != want) fail("store is not the lane's output pixel", c);
                    if (written[off / 16]++) fail("output element written twice", c);
                }
            for (int tdw = 0; tdw < 4; ++tdw) {
                const unsigned m = upb_dword_mask(g, it.k, tdw);
                for (int b = 0; b < 4; ++b) {
                    const bool real = 16 * it.k + 4 * tdw + b < c.C;
                    if ((((m >> (8 * b)) & 0xffu) == 0xffu) != real || (((m >> (8 * b)) & 0xffu) != 0u) != real) fail("channel mask", c);
                }
            }
            second += round == 1;
            i += threads;
            if (i >= g.items) break;
            it = upb_next(g, it);
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output element not written", c);
    if (print) printf("case %d,%d,%d,%d,%d: items %u blocks %u second-items %ld\n", c.N, c.H, c.W, c.C, c.up, g.items, blocks, second);
    return loads;
}

// upb_requant against S 2^e rounded half to even in double (nearbyint in the default rounding mode), then ReLU and clamp
static void check_rounding() {
    for (int up : {2, 4})
        for (int shift = -kUpbMaxShift; shift <= kUpbMaxShift; ++shift)
            for (int relu = 0; relu < 2; ++relu) {
                const UpbRound r = upb_round(up, shift, relu);
                const int lim = 128 * 4 * up * up;
                if (r.rsh > 14 || r.lsh > 4 || (r.rsh > 0 && r.lsh > 0)) { printf("shift amounts: up %d shift %d\n", up, shift); exit(1); }
                for (int S = -lim; S <= lim; ++S) {
                    double v = std::nearbyint(std::ldexp((double)S, shift - 2 * (upb_log2(up) + 1)));
                    if (relu && v < 0) v = 0;
                    v = v < -128 ? -128 : (v > 127 ? 127 : v);
                    if (r.rsh > 0 && (S + r.bias + 1 > 32767 || S + r.bias < -32768)) { printf("int16 overflow: S %d\n", S); exit(1); }
                    if (upb_requant(S, r) != (int)v) {
                        printf("rounding: up %d shift %d relu %d S %d: %d, expected %d\n", up, shift, relu, S, upb_requant(S, r), (int)v);
                        exit(1);
                    }
                }
            }
    // the guards of upb_args: 0 fine, -1 invalid, -4 not taken
    if (upb_args(1, 1, 1, 1, 16, 2, 0) != 0 || upb_args(0, 1, 1, 1, 16, 2, 0) != 0 || upb_args(-1, 1, 1, 1, 16, 2, 0) != -1 ||
        upb_args(1, 0, 1, 1, 16, 2, 0) != -1 || upb_args(1, 1, 1, 17, 16, 2, 0) != -1 || upb_args(1, 1, 1, 1, 24, 2, 0) != -1 ||
        upb_args(1, 1, 1, 1, 16, 3, 0) != -4 || upb_args(1, 1, 1, 1, 16, 2, 9) != -4 || upb_args(1, 1, 1, 1, 16, 4, -9) != -4 ||
        upb_args(1, 8192, 8192, 1, 16, 2, 0) != -4 || upb_args(1, 4096, 8191, 16, 16, 2, 0) != 0 ||
        upb_args(2147483647, 2147483647, 2147483647, 1, 2147483632, 4, 0) != -4) {
        printf("upb_args\n");
        exit(1);
    }
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
        const int planes[][2] = {{1, 1}, {1, 5}, {3, 2}, {2, 3}, {7, 9}, {8, 8}, {33, 47}};
        const int chans[] = {1, 16, 19, 33, 80};
        for (int up : {2, 4})
            for (int N : {1, 3})
                for (const auto& pl : planes)
                    for (int C : chans) cases.push_back(Case{N, pl[0], pl[1], C, up});
        cases.push_back(Case{1, 592, 592, 48, 2});           // 1 051 392 items: past 4096 x 256 lanes, a second item per lane
        cases.push_back(Case{1, 592, 592, 48, 4});
        for (int lvl = 0; lvl < 4; ++lvl)                    // UNet(base_width 32, depth 4) at 224 x 224, batch 8: the decoder's four launches
            cases.push_back(Case{8, 14 << lvl, 14 << lvl, 256 >> lvl, 2});
        cases.push_back(Case{4, 8, 8, 16, 2});               // UNet(base_width 8, depth 2) at 32 x 32, batch 4 (the GPU tests)
        cases.push_back(Case{4, 16, 16, 8, 2});
    }
    check_rounding();
    long total = 0;
    for (const Case& c : cases) total += run(c, true);
    printf("ok, %ld loads checked\n", total);
    return 0;
}
