// deconv_geom_check.cpp -- walks fq_deconv_i8_geom.h on the host, lane by lane, the way deconv_i8_kernel uses it.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pytorch-quantity_amd/csrc \
//       scripts/deconv_geom_check.cpp -o deconv_geom_check && ./deconv_geom_check
//
// For every case (a built-in list of the shapes of tests/test_gpu_deconv_i8.py, the launch shapes of UNet(up="deconv") and a launch
// with more items than the capped grid has workgroups; or the cases given as arguments, N,H,W,C,K,R,S,sh,sw,ph,pw,oph,opw each:
// tests/test_deconv_plan_cpu.py passes every case of the GPU tests) and every lane of every workgroup it asserts that
//   * every operand load is 16 bytes, aligned, inside x or the packed weights -- or the out-of-range offset;
//   * every 16-byte store is aligned and inside q, and every byte of q is written exactly once: the rows and columns that exist
//     only through output_padding and the phases without a tap included;
//   * the taps a lane accumulates for an output pixel are exactly the (ih, iw, r, s) of the rule in include/fq.h, each once, and
//     the weight chunk it pairs with an activation chunk holds that tap (against an index-valued pack made by the header's rule);
//   * the digit walk agrees with the division at every step;
//   * fq_deconv2d_i8_supported's table, row by row, and the guard's order of verdicts.
// CPU only; prints "deconv_geom_check: OK ..." and returns 0, or aborts on the first failure.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "fq_deconv_i8_geom.h"

using namespace fq;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::abort();                                                               \
        }                                                                               \
    } while (0)

struct Case {
    int N, H, W, C, K, R, S, sh, sw, ph, pw, oph, opw;
};

static long g_loads = 0, g_stores = 0, g_taps = 0, g_steps = 0;

// the packed weights hold, per 16-byte chunk, the (r, s, c / 16) it was made from and per row the k: built by the rule of fq.h
struct WChunk {
    int k, r, s, cc;
};

static void walk_case(const Case& t) {
    int launch = 0;
    CHECK(dc_guard(16, 16, 16, 16, dc_pad16(t.C), dc_pad16(t.K), -128, 127, t.N, t.H, t.W, t.C, t.K, t.R, t.S, t.sh, t.sw, t.ph, t.pw, t.oph,
                   t.opw, 7, 0, &launch) == kDcOk && launch == 1);
    const DcGeom g = dc_geom(t.N, t.H, t.W, t.C, t.K, t.R, t.S, t.sh, t.sw, t.ph, t.pw, t.oph, t.opw);
    CHECK(g.P == (t.H - 1) * t.sh - 2 * t.ph + t.R + t.oph && g.Q == (t.W - 1) * t.sw - 2 * t.pw + t.S + t.opw);
    CHECK(g.blocks >= 1 && g.blocks <= (unsigned)kDcMaxBlocks && g.blocks <= g.items);
    CHECK(g.w_bytes == dc_packed_bytes(t.C, t.K, t.R, t.S) && g.w_bytes % 16 == 0);
    CHECK(g.KW == 32 || g.KW == 64);

    // the pack by the header's words
    std::vector<WChunk> wpack(g.w_bytes / 16, WChunk{-1, -1, -1, -1});
    {
        size_t at = 0;
        for (int fh = 0; fh < t.sh; ++fh)
            for (int fw = 0; fw < t.sw; ++fw) {
                const int a = (fh + t.ph) % t.sh, b = (fw + t.pw) % t.sw;
                const int Th = a < t.R ? (t.R - a + t.sh - 1) / t.sh : 0, Tw = b < t.S ? (t.S - b + t.sw - 1) / t.sw : 0;
                const DcPhase p = dc_phase(g, (unsigned)(fh * t.sw + fw));
                CHECK(p.woff == at * 16 && p.h.T == Th && p.w.T == Tw && p.h.a == a && p.w.a == b);
                for (int k = 0; k < g.Kpad; ++k)
                    for (int th = 0; th < Th; ++th)
                        for (int tw = 0; tw < Tw; ++tw)
                            for (int cc = 0; cc < g.c16; ++cc) wpack[at++] = WChunk{k, a + t.sh * th, b + t.sw * tw, cc};
            }
        CHECK(at == wpack.size());
    }

    std::vector<unsigned char> written(g.q_bytes, 0);
    for (unsigned blk = 0; blk < g.blocks; ++blk) {
        for (int tid = 0; tid < kDcBlock; ++tid) {
            const int lane = tid & 63, l32 = lane & 31, half = lane >> 5, wave = tid >> 6;
            unsigned item = blk;
            const unsigned slot = (unsigned)(wave * 32 + l32);
            DcWalk s = dc_walk_begin(g, item, slot);
            for (; item < g.items; item += g.blocks) {
                ++g_steps;
                const DcWalk ref = dc_walk_begin(g, item, slot);                       // the walk against the division
                CHECK(ref.f == s.f && ref.kb == s.kb && ref.mt == s.mt && ref.n == s.n && ref.j == s.j && ref.i == s.i);
                CHECK(s.f < g.F && s.kb < g.KB && s.mt < g.MT && s.j < g.PJ && s.i < g.QJ);
                const DcPhase p = dc_phase(g, s.f);
                const int k0 = (int)s.kb * g.KW;
                const bool ok = dc_pix_ok(g, p, s);
                const int oh = p.h.f + g.sh * (int)s.j, ow = p.w.f + g.sw * (int)s.i;
                std::set<std::tuple<int, int, int, int>> taps;                          // (ih, iw, r, s), this half's chunks
                DcChunk c = dc_chunk_begin();
                if (half) dc_chunk_next(g, p, c);
                const int steps = (p.chunks + 1) / 2;
                for (int st = 0; st < steps; ++st) {
                    CHECK(c.ch == 2 * st + half);
                    for (int a = 0; a < g.KW / 32; ++a) {                              // the weights: whatever the pixel is
                        const int k = k0 + 32 * a + l32;
                        const unsigned wo = dc_w_off(g, p, k, c.ch);
                        ++g_loads;
                        if (k >= g.Kpad || c.ch >= p.chunks) { CHECK(wo == kDcOutOfRange); continue; }
                        CHECK(wo % 16 == 0 && (unsigned long)wo + 16 <= g.w_bytes);
                        const WChunk& wc = wpack[wo / 16];
                        CHECK(wc.k == k && wc.r == p.h.a + g.sh * c.th && wc.s == p.w.a + g.sw * c.tw && wc.cc == c.cc);
                    }
                    const unsigned xo = dc_x_off(g, p, s, ok, c);
                    ++g_loads;
                    if (xo != kDcOutOfRange) {
                        CHECK(ok && xo % 16 == 0 && (unsigned long)xo + 16 <= g.x_bytes && c.ch < p.chunks);
                        const int r = p.h.a + g.sh * c.th, sx = p.w.a + g.sw * c.tw;
                        CHECK(c.ch == (c.th * p.w.T + c.tw) * g.c16 + c.cc && r < g.R && sx < g.S);
                        const unsigned pix = xo / (unsigned)g.Cpad;
                        const int iw = (int)(pix % (unsigned)g.W), ih = (int)((pix / (unsigned)g.W) % (unsigned)g.H);
                        CHECK(pix / (unsigned)(g.W * g.H) == s.n && xo % (unsigned)g.Cpad == 16u * (unsigned)c.cc);
                        CHECK(oh + g.ph - r == ih * g.sh && ow + g.pw - sx == iw * g.sw);      // the rule
                        if (c.cc == 0) { CHECK(taps.insert({ih, iw, r, sx}).second); ++g_taps; }
                    }
                    dc_chunk_next(g, p, c);
                    dc_chunk_next(g, p, c);
                }
                if (ok && half == 0) {
                    // both halves together hold every tap of the rule: half 1 walks the odd chunks of the same pixel
                    std::set<std::tuple<int, int, int, int>> all;
                    DcChunk e = dc_chunk_begin();
                    for (int ch = 0; ch < p.chunks; ++ch, dc_chunk_next(g, p, e)) {
                        const int ih = (int)s.j + p.h.d - e.th, iw = (int)s.i + p.w.d - e.tw;
                        if (e.cc == 0 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) all.insert({ih, iw, p.h.a + g.sh * e.th, p.w.a + g.sw * e.tw});
                    }
                    std::set<std::tuple<int, int, int, int>> rule;
                    for (int r = 0; r < g.R; ++r)
                        for (int sx = 0; sx < g.S; ++sx) {
                            const int nh = oh + g.ph - r, nw = ow + g.pw - sx;
                            if (nh < 0 || nw < 0 || nh % g.sh || nw % g.sw) continue;
                            if (nh / g.sh < g.H && nw / g.sw < g.W) rule.insert({nh / g.sh, nw / g.sw, r, sx});
                        }
                    CHECK(all == rule);
                }
                if (ok) {
                    CHECK(oh < g.P && ow < g.Q && s.n < (unsigned)g.N);
                    for (int a = 0; a < g.KW / 32; ++a) {
                        const int kc = k0 + 32 * a + 16 * half;
                        if (kc >= g.Kpad) continue;
                        const unsigned qo = dc_q_off(g, p, s, kc);
                        CHECK(qo % 16 == 0 && (unsigned long)qo + 16 <= g.q_bytes);
                        CHECK(qo == (((s.n * (unsigned)g.P + (unsigned)oh) * (unsigned)g.Q + (unsigned)ow) * (unsigned)g.Kpad + (unsigned)kc));
                        for (int b = 0; b < 16; ++b) CHECK(written[qo + b]++ == 0);
                        ++g_stores;
                    }
                }
                dc_walk_step(g, s);
            }
        }
    }
    for (size_t b = 0; b < written.size(); ++b) CHECK(written[b] == 1);
    // the accumulator's channel map: the four runs of a half-wave and its partner's tile the 32 channels
    std::vector<int> seen(32, 0);
    for (int half = 0; half < 2; ++half)
        for (int e = 0; e < 16; ++e) {
            CHECK(dc_acc_channel(e, half) == 8 * (e >> 2) + 4 * half + (e & 3));
            ++seen[dc_acc_channel(e, half)];
        }
    for (int k = 0; k < 32; ++k) CHECK(seen[k] == 1);
}

static void check_supported() {
    struct Row {
        int C, K, groups, R, S, sh, sw, ph, pw, oph, opw, dh, dw, lo, hi, want;
    };
    const Row rows[] = {
        {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 1},   {8, 8, 1, 4, 4, 2, 2, 1, 1, 0, 0, 1, 1, 1, 16, 1},
        {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1},   {8, 8, 1, 8, 8, 4, 4, 7, 7, 3, 3, 1, 1, 16, 16, 1},
        {8, 8, 1, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 5, 5, 1},   {8, 8, 1, 2, 3, 2, 1, 0, 0, 0, 0, 1, 1, 5, 5, 1},
        {8, 8, 1, 2, 2, 4, 4, 0, 0, 3, 3, 1, 1, 5, 5, 1},   {8, 8, 2, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 2, 1, 7, 7, 0},   {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 2, 7, 7, 0},
        {8, 8, 1, 9, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 2, 9, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 5, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 2, 2, 2, 5, 0, 0, 0, 0, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 2, 2, 2, 0, 0, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 2, 2, 2, 2, 0, 2, 0, 0, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 2, 2, 0, 0, 2, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 2, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 0, 7, 0},   {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 17, 0},
        {8, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 8, 7, 0},   {0, 8, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},
        {8, 0, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 0, 2, 2, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},
        {8, 8, 1, 2, 2, 0, 2, 0, 0, 0, 0, 1, 1, 7, 7, 0},   {8, 8, 1, 2, 2, 2, 2, -1, 0, 0, 0, 1, 1, 7, 7, 0},
        // the accumulator bound: 64 taps x C x 2^14 + 2^16 + (255 << 16) against 2^31 - 1
        {2031, 8, 1, 8, 8, 1, 1, 0, 0, 0, 0, 1, 1, 16, 16, 1}, {2032, 8, 1, 8, 8, 1, 1, 0, 0, 0, 0, 1, 1, 16, 16, 0},
        {8124, 8, 1, 8, 8, 2, 2, 0, 0, 0, 0, 1, 1, 16, 16, 1}, {8128, 8, 1, 8, 8, 2, 2, 0, 0, 0, 0, 1, 1, 16, 16, 0},
    };
    for (const Row& r : rows)
        CHECK(dc_supported(r.C, r.K, r.groups, r.R, r.S, r.sh, r.sw, r.ph, r.pw, r.oph, r.opw, r.dh, r.dw, r.lo, r.hi) == (r.want != 0));
    for (const Row& r : rows) {                                                         // the bound, recomputed
        if (r.C < 1 || r.K < 1 || r.R < 1 || r.S < 1 || r.sh < 1 || r.sw < 1 || r.hi > 16 || r.hi < 1) continue;
        const long acc = (long)((r.R + r.sh - 1) / r.sh) * ((r.S + r.sw - 1) / r.sw) * r.C * 16384L + 65536L + (255L << r.hi);
        if (r.want) CHECK(acc < 0x7fffffffL);
    }
    // the guard: scalars before pointers, N == 0 before pointers
    int launch = 1;
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 0, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcOk && launch == 0);
    CHECK(dc_guard(0, 16, 16, 16, 16, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid && launch == 0);
    CHECK(dc_guard(16, 16, 16, 24, 16, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 1, 4, 4, 8, 8, 9, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcUnsupported);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 17, 0, &launch) == kDcUnsupported);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, &launch) == kDcUnsupported);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 121, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, 1, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 128, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, -1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 16, -128, 127, 1, 0, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 32, 16, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(0, 0, 0, 0, 16, 32, -128, 127, 1, 4, 4, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcInvalid);
    CHECK(dc_guard(16, 16, 16, 16, 16, 16, -128, 127, 1, 1, 1, 8, 8, 3, 3, 1, 1, 2, 2, 0, 0, 7, 0, &launch) == kDcInvalid);   // P = -1
    CHECK(dc_guard(16, 16, 16, 16, 16, 16, -128, 127, 4096, 1024, 1024, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcUnsupported);
    CHECK(dc_guard(16, 16, 16, 16, 16, 16, -128, 127, 64, 1024, 1024, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0, &launch) == kDcUnsupported);   // q >= 2^30
}

int main(int argc, char** argv) {
    check_supported();
    if (argc > 1) {                                                                     // cases given as N,H,W,C,K,R,S,sh,sw,ph,pw,oph,opw
        for (int a = 1; a < argc; ++a) {
            Case t;
            if (std::sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", &t.N, &t.H, &t.W, &t.C, &t.K, &t.R, &t.S, &t.sh, &t.sw, &t.ph,
                            &t.pw, &t.oph, &t.opw) != 13) {
                std::fprintf(stderr, "bad case: %s\n", argv[a]);
                return 2;
            }
            walk_case(t);
            const DcGeom g = dc_geom(t.N, t.H, t.W, t.C, t.K, t.R, t.S, t.sh, t.sw, t.ph, t.pw, t.oph, t.opw);
            std::printf("case %s: items %u blocks %u KW %d\n", argv[a], g.items, g.blocks, g.KW);
        }
        std::printf("deconv_geom_check: OK  %d cases, %ld lane steps, %ld loads, %ld taps, %ld stores\n", argc - 1, g_steps, g_loads, g_taps,
                    g_stores);
        return 0;
    }
    const Case cases[] = {
        // tests/test_gpu_deconv_i8.py: planes 1x1, 2x3, 5x4, 8x8; (C, K) pairs; the seven (k, s, p, op); the rectangle
        {1, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0},     {3, 2, 3, 3, 5, 3, 3, 2, 2, 1, 1, 1, 1},    {1, 5, 4, 16, 16, 4, 4, 2, 2, 1, 1, 0, 0},
        {3, 8, 8, 17, 33, 3, 3, 1, 1, 1, 1, 0, 0},   {1, 5, 4, 40, 64, 4, 4, 4, 4, 0, 0, 0, 0},  {3, 2, 3, 3, 33, 2, 2, 4, 4, 0, 0, 0, 0},
        {1, 8, 8, 17, 5, 5, 5, 3, 3, 2, 2, 1, 1},    {3, 5, 4, 16, 64, 2, 3, 2, 1, 0, 0, 0, 0},  {1, 1, 1, 40, 1, 5, 5, 3, 3, 2, 2, 1, 1},
        {3, 8, 8, 1, 16, 2, 2, 2, 2, 0, 0, 0, 0},    {1, 2, 3, 40, 33, 3, 3, 2, 2, 1, 1, 1, 1},  {3, 5, 4, 3, 5, 4, 4, 2, 2, 1, 1, 0, 0},
        {1, 8, 8, 16, 16, 2, 2, 4, 4, 0, 0, 3, 3},   {1, 1, 1, 17, 64, 3, 3, 2, 2, 1, 1, 1, 1},  {3, 5, 4, 1, 1, 8, 8, 4, 4, 7, 7, 3, 3},
        // more items than the capped grid has workgroups (the digit walk with both carries); an odd chunk count (3 taps x 1)
        {3, 33, 35, 5, 70, 3, 3, 2, 2, 1, 1, 1, 1},  {8, 32, 33, 3, 70, 2, 2, 4, 4, 0, 0, 1, 2}, {1, 7, 5, 16, 16, 3, 1, 1, 1, 1, 0, 0, 0},
        // smoke()
        {2, 4, 5, 5, 3, 3, 3, 2, 2, 1, 1, 1, 1},
        // UNet(base_width 8, depth 2, up="deconv") at 32x32, batch 2: kernels 2, 3, 4
        {2, 8, 8, 32, 16, 2, 2, 2, 2, 0, 0, 0, 0},   {2, 16, 16, 16, 8, 2, 2, 2, 2, 0, 0, 0, 0}, {2, 8, 8, 32, 16, 3, 3, 2, 2, 1, 1, 1, 1},
        {2, 16, 16, 16, 8, 3, 3, 2, 2, 1, 1, 1, 1},  {2, 8, 8, 32, 16, 4, 4, 2, 2, 1, 1, 0, 0},  {2, 16, 16, 16, 8, 4, 4, 2, 2, 1, 1, 0, 0},
        // UNet(base_width 32, depth 4, up="deconv") at 224x224 (scripts/deconv_cost.py), one image: 14, 28, 56, 112 planes
        {1, 14, 14, 512, 256, 2, 2, 2, 2, 0, 0, 0, 0}, {1, 28, 28, 256, 128, 4, 4, 2, 2, 1, 1, 0, 0},
        {1, 56, 56, 128, 64, 2, 2, 2, 2, 0, 0, 0, 0},  {1, 112, 112, 64, 32, 4, 4, 2, 2, 1, 1, 0, 0},
    };
    int n = 0;
    bool capped = false, odd = false, empty = false;
    for (const Case& t : cases) {
        walk_case(t);
        const DcGeom g = dc_geom(t.N, t.H, t.W, t.C, t.K, t.R, t.S, t.sh, t.sw, t.ph, t.pw, t.oph, t.opw);
        capped = capped || g.items > g.blocks;
        for (unsigned f = 0; f < g.F; ++f) {
            const DcPhase p = dc_phase(g, f);
            odd = odd || (p.chunks & 1);
            empty = empty || p.chunks == 0;
        }
        ++n;
    }
    CHECK(capped && odd && empty);
    std::printf("deconv_geom_check: OK  %d cases, %ld lane steps, %ld loads, %ld taps, %ld stores\n", n, g_steps, g_loads, g_taps, g_stores);
    return 0;
}
