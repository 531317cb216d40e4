// Host check of the pixel shuffle / unshuffle kernel's guards, launch geometry and address arithmetic
// (csrc/fq_pixel_shuffle_i8_geom.h), after the pattern of shuffle_geom_check.cpp: every lane of every launch is walked with the
// kernel's own functions -- the same launch size, the same stride loop and digit walk, the same load and store offsets, the same
// v_perm_b32 network (ps_perm computes the instruction's result on the host) -- and the walk asserts that
//   * every load is aligned (16 bytes in the aligned family, 4 in the general one) and inside the source;
//   * every store is an aligned 16-byte chunk inside the output, and every chunk is written exactly once;
//   * every output byte comes from the source byte the index rule of include/fq.h names, computed here from the output address
//     alone; bytes at or above the real width come from nowhere (the padding mask): they are zero without a read;
//   * the digit walk agrees with the division at every step;
//   * the guard returns the documented code for every row of its table (always run first).
// The aligned family's network works on real dwords, so it is run four times on a source whose byte at address a holds byte p of
// a (p = 0 .. 3): together the four results name the 32-bit address each output byte came from.
//   c++ -O2 -std=c++17 -o pixel_shuffle_geom_check scripts/pixel_shuffle_geom_check.cpp    (tests add -fsanitize=address,undefined)
//   ./pixel_shuffle_geom_check                           the built-in shape list
//   ./pixel_shuffle_geom_check N,H,W/C,r,inverse ...     these cases instead; tests pass the GPU tests' and the model's list
// One line per case: "case N,H,W/C,r,inverse: family F items I blocks B passes P", then "ok, <bytes> bytes checked".  Exit status
// 1 at the first violation.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_pixel_shuffle_i8_geom.h"

using namespace fq;

struct Case { int N, H, W, C, r, inv; std::string text; };

static void fail(const char* what, const Case& c) {
    printf("%s: %s\n", what, c.text.c_str());
    exit(1);
}

// the index rule, from the output byte address alone: the source byte address, or -1 for a padding channel
static long rule(const Case& c, long out_addr) {
    const long r = c.r, deep = ps_pad16(c.C * c.r * c.r), shal = ps_pad16(c.C);
    if (!c.inv) {
        const long ch = out_addr % shal, pix = out_addr / shal;
        const long ww = pix % (c.W * r), rest = pix / (c.W * r), hh = rest % (c.H * r), n = rest / (c.H * r);
        if (ch >= c.C) return -1;
        const long h = hh / r, i = hh % r, w = ww / r, j = ww % r;
        return ((n * c.H + h) * c.W + w) * deep + ch * r * r + i * r + j;
    }
    const long co = out_addr % deep, pix = out_addr / deep;
    const long w = pix % c.W, rest = pix / c.W, h = rest % c.H, n = rest / c.H;
    if (co >= (long)c.C * r * r) return -1;
    const long ch = co / (r * r), q = co % (r * r), i = q / r, j = q % r;
    return ((n * c.H * r + h * r + i) * (c.W * r) + w * r + j) * shal + ch;
}

template <int Q>
static void network(const Case& c, const PsV4 (&in)[Q], PsV4 (&out)[Q]);
template <>
void network<4>(const Case& c, const PsV4 (&in)[4], PsV4 (&out)[4]) {
    if (c.inv) ps_net2_s2d(in, out);
    else ps_net2_d2s(in, out);
}
template <>
void network<16>(const Case&, const PsV4 (&in)[16], PsV4 (&out)[16]) { ps_net4(in, out); }

template <int R>
static void walk_aligned_item(const Case& c, const PsGeom& g, unsigned item, const PsWalk& s, long src_bytes, long out_bytes,
                              std::vector<unsigned char>& written, long& checked) {
    constexpr int Q = R * R;
    long load[Q], store[Q];
    for (int q = 0; q < Q; ++q) {
        const size_t deep = ps_deep_off(g, item, q, R), shal = ps_shallow_off(g, s, q / R, q % R, R);
        load[q] = (long)(c.inv ? shal : deep);
        store[q] = (long)(c.inv ? deep : shal);
        if (load[q] % 16 || load[q] < 0 || load[q] + 16 > src_bytes) fail("dwordx4 load outside the source or unaligned", c);
        if (store[q] % 16 || store[q] < 0 || store[q] + 16 > out_bytes) fail("dwordx4 store outside the output or unaligned", c);
    }
    long from[Q][16];
    for (int q = 0; q < Q; ++q)
        for (int b = 0; b < 16; ++b) from[q][b] = 0;
    for (int p = 0; p < 4; ++p) {
        PsV4 in[Q], out[Q];
        for (int q = 0; q < Q; ++q)
            for (int d = 0; d < 4; ++d) {
                unsigned v = 0;
                for (int e = 0; e < 4; ++e) v |= (unsigned)(((unsigned long)(load[q] + 4 * d + e) >> (8 * p)) & 0xffu) << (8 * e);
                in[q].d[d] = v;
            }
        network<Q>(c, in, out);
        for (int q = 0; q < Q; ++q)
            for (int b = 0; b < 16; ++b) from[q][b] |= (long)((out[q].d[b / 4] >> (8 * (b % 4))) & 0xffu) << (8 * p);
    }
    for (int q = 0; q < Q; ++q)
        for (int b = 0; b < 16; ++b) {
            if (from[q][b] != rule(c, store[q] + b)) fail("output byte is not the byte the index rule names", c);
            if (written[(size_t)store[q] + b]++) fail("output byte written twice", c);
            ++checked;
        }
}

static long run(const Case& c, bool print) {
    int launch = 0;
    const int deep = ps_pad16(c.C * c.r * c.r), shal = ps_pad16(c.C);
    if (ps_guard(64, c.inv ? shal : deep, 128, c.inv ? deep : shal, c.C, c.r, c.inv, c.N, c.H, c.W, &launch) != kPsOk || !launch)
        fail("a case the entry point refuses", c);
    const PsGeom g = ps_geom(c.C, c.r, c.inv, c.N, c.H, c.W);
    const long lo_pix = (long)c.N * c.H * c.W;
    const long src_bytes = c.inv ? lo_pix * c.r * c.r * shal : lo_pix * deep;
    const long out_bytes = c.inv ? lo_pix * deep : lo_pix * c.r * c.r * shal;
    if (g.family != kPsAligned && g.family != kPsGeneral) fail("no family", c);
    if ((g.family == kPsAligned) != (c.r != 3 && c.C % 16 == 0)) fail("the wrong family", c);
    if (g.blocks < 1 || g.blocks > (unsigned)kPsMaxBlocks || g.stride != g.blocks * (unsigned)kPsBlock) fail("launch size", c);
    if ((unsigned long)g.blocks * kPsBlock < g.items && g.blocks != (unsigned)kPsMaxBlocks) fail("too few workgroups below the cap", c);
    if (((unsigned long)g.drow * g.Wd + g.dw) * g.CH + g.dk != g.stride || g.dk >= g.CH || g.dw >= g.Wd) fail("the stride's digits", c);
    if ((unsigned long)g.items + g.stride > 0xffffffffUL) fail("32-bit item arithmetic wraps", c);
    const long per_item = g.family == kPsAligned ? 16l * c.r * c.r : 16l;
    if ((long)g.items * per_item != out_bytes) fail("the items do not cover the output", c);
    const unsigned passes = (g.items + g.stride - 1) / g.stride;
    if (print) printf("case %s: family %d items %u blocks %u passes %u\n", c.text.c_str(), g.family, g.items, g.blocks, passes);
    std::vector<unsigned char> written((size_t)out_bytes, 0);
    long checked = 0;
    for (unsigned blk = 0; blk < g.blocks; ++blk)
        for (unsigned tid = 0; tid < (unsigned)kPsBlock; ++tid) {
            unsigned item = blk * (unsigned)kPsBlock + tid;
            if (item >= g.items) continue;
            PsWalk s = ps_walk_begin(g, item);
            for (; item < g.items; item += g.stride) {
                const PsWalk want = ps_walk_begin(g, item);
                if (s.row != want.row || s.w != want.w || s.k != want.k) fail("the digit walk left the division", c);
                if (g.family == kPsAligned) {
                    if (c.r == 2) walk_aligned_item<2>(c, g, item, s, src_bytes, out_bytes, written, checked);
                    else walk_aligned_item<4>(c, g, item, s, src_bytes, out_bytes, written, checked);
                } else {
                    const long store = 16l * item;
                    if (store + 16 > out_bytes) fail("dwordx4 store outside the output", c);
                    for (int b = 0; b < 16; ++b) {
                        const long want_src = rule(c, store + b);
                        long got = -1;
                        if (ps_gen_real(g, s, b)) {
                            got = (long)ps_gen_src(g, s, b, c.r);
                            const long word = got & ~3l;
                            if (got < 0 || word + 4 > src_bytes) fail("dword load outside the source", c);
                        }
                        if ((got < 0) != (want_src < 0)) fail("the padding mask", c);
                        if (got != want_src) fail("output byte is not the byte the index rule names", c);
                        if (written[(size_t)store + b]++) fail("output byte written twice", c);
                        ++checked;
                    }
                }
                ps_walk_step(g, s);
            }
        }
    for (unsigned char v : written)
        if (v != 1) fail("output byte not written", c);
    return checked;
}

static Case make(int N, int H, int W, int C, int r, int inv) {
    Case c;
    c.N = N; c.H = H; c.W = W; c.C = C; c.r = r; c.inv = inv;
    c.text = std::to_string(N) + "," + std::to_string(H) + "," + std::to_string(W) + "/" + std::to_string(C) + "," + std::to_string(r) +
             "," + std::to_string(inv);
    return c;
}

// the guard's table: (x, Cpad_in, y, Cpad_out, C, r, inverse, N, H, W) -> code, launch
static void guards() {
    struct Row { const char* what; uintptr_t x; int cin; uintptr_t y; int cout, C, r, inv, N, H, W, code, launch; };
    const uintptr_t P = 4096, Q = 8192;
    const int big = 1 << 30;
    const Row rows[] = {
        {"shuffle, RGB head", P, 16, Q, 16, 3, 2, 0, 1, 2, 2, kPsOk, 1},
        {"unshuffle", P, 16, Q, 64, 16, 2, 1, 2, 5, 4, kPsOk, 1},
        {"r = 3, C = 17", P, 160, Q, 32, 17, 3, 0, 1, 1, 1, kPsOk, 1},
        {"the widest row", P, 65536, Q, 4096, 4096, 4, 0, 1, 1, 1, kPsOk, 1},
        {"N == 0, no pointers", 0, 16, 0, 16, 3, 2, 0, 0, 2, 2, kPsOk, 0},
        {"N == 0, a wrong Cpad", 0, 32, 0, 16, 3, 2, 0, 0, 2, 2, kPsInvalid, 0},
        {"N < 0", P, 16, Q, 16, 3, 2, 0, -1, 2, 2, kPsInvalid, 0},
        {"H < 1", P, 16, Q, 16, 3, 2, 0, 1, 0, 2, kPsInvalid, 0},
        {"W < 1", P, 16, Q, 16, 3, 2, 0, 1, 2, 0, kPsInvalid, 0},
        {"C < 1", P, 16, Q, 16, 0, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"inverse == 2", P, 16, Q, 16, 3, 2, 2, 1, 2, 2, kPsInvalid, 0},
        {"inverse == -1", P, 16, Q, 16, 3, 2, -1, 1, 2, 2, kPsInvalid, 0},
        {"r == 1", P, 16, Q, 16, 3, 1, 0, 1, 2, 2, kPsUnsupported, 0},
        {"r == 5", P, 80, Q, 16, 3, 5, 0, 1, 2, 2, kPsUnsupported, 0},
        {"r == 0", P, 16, Q, 16, 3, 0, 0, 1, 2, 2, kPsUnsupported, 0},
        {"C r^2 > 65536", P, 65552, Q, 16400, 16385, 2, 0, 1, 1, 1, kPsUnsupported, 0},
        {"wrong Cpad_in", P, 32, Q, 16, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"wrong Cpad_out", P, 16, Q, 32, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"the other direction's Cpads", P, 64, Q, 16, 16, 2, 1, 1, 2, 2, kPsInvalid, 0},
        {"an output of 2^31 bytes", P, 16, Q, 16, 3, 2, 0, big / 16 / 2, 1, 1, kPsUnsupported, 0},
        {"a source of 2^31 bytes", P, 64, Q, 16, 16, 2, 0, big / 64 * 2, 1, 1, kPsUnsupported, 0},
        {"N H W alone past 2^31", P, 16, Q, 16, 3, 2, 0, 1, 1 << 20, 1 << 20, kPsUnsupported, 0},
        {"N H W past 2^47", P, 16, Q, 16, 3, 2, 0, 1 << 16, 1 << 16, 1 << 16, kPsUnsupported, 0},
        {"just below the limit", P, 16, Q, 16, 3, 2, 0, big / 16 / 2 - 1, 1, 1, kPsOk, 1},
        {"null x", 0, 16, Q, 16, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"null y", P, 16, 0, 16, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"misaligned x", P + 4, 16, Q, 16, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"misaligned y", P, 16, Q + 8, 16, 3, 2, 0, 1, 2, 2, kPsInvalid, 0},
        {"a wrong scalar beats a null pointer", 0, 16, 0, 16, 3, 7, 0, 1, 2, 2, kPsUnsupported, 0},
    };
    for (const Row& t : rows) {
        int launch = -1;
        const int code = ps_guard(t.x, t.cin, t.y, t.cout, t.C, t.r, t.inv, t.N, t.H, t.W, &launch);
        if (code != t.code || launch != t.launch) {
            printf("guard row '%s': code %d launch %d, want %d %d\n", t.what, code, launch, t.code, t.launch);
            exit(1);
        }
        if ((ps_family(t.C, t.r, t.inv) != 0) != (t.C >= 1 && t.r >= 2 && t.r <= 4 && (t.inv == 0 || t.inv == 1) && (long)t.C * t.r * t.r <= kPsMaxDeepC)) {
            printf("guard row '%s': ps_family disagrees\n", t.what);
            exit(1);
        }
    }
}

int main(int argc, char** argv) {
    guards();
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        int N, H, W, C, r, inv;
        if (sscanf(argv[a], "%d,%d,%d/%d,%d,%d", &N, &H, &W, &C, &r, &inv) != 6) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(make(N, H, W, C, r, inv));
    }
    if (cases.empty()) {
        const int planes[][2] = {{1, 1}, {2, 3}, {5, 4}, {8, 8}, {1, 7}};
        const int widths[] = {1, 3, 4, 15, 16, 17, 32, 48, 64, 100};
        for (int inv = 0; inv < 2; ++inv)
            for (int r = 2; r <= 4; ++r) {
                for (const auto& p : planes)
                    for (int C : widths)
                        for (int N : {1, 3}) cases.push_back(make(N, p[0], p[1], C, r, inv));
            }
        // more items than 2048 x 256 lanes: a lane takes a second item (and, in the general shuffle, a part of them a third).  The
        // GPU tests' two large launches are these with the directions exchanged; the tests pass them as arguments.
        cases.push_back(make(1, 96, 96, 1024, 2, 1));
        cases.push_back(make(1, 250, 240, 17, 3, 0));
        cases.push_back(make(1, 1, 1, 4096, 4, 0));                           // the widest row
        cases.push_back(make(1, 1, 2, 7281, 3, 1));                           // ... of r = 3 (65529 real channels)
    }
    long total = 0;
    for (const Case& c : cases) total += run(c, argc > 1);
    printf("ok, %ld bytes checked\n", total);
    return 0;
}
