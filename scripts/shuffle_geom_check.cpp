// Host check of the channel shuffle / slice kernel's address arithmetic (csrc/fq_shuffle_i8_geom.h), after the pattern of
// concat_geom_check.cpp: every address a lane may touch -- a 16-byte stage load, its LDS destination, an LDS or global byte
// read, a 16-byte store -- lies inside its tensor and is aligned, every output byte is written exactly once, and every output
// byte comes from the channel the rule names (bytes j >= C from nowhere: they are zero).
//   c++ -O2 -std=c++17 -o shuffle_geom_check scripts/shuffle_geom_check.cpp      (tests add -fsanitize=address,undefined)
//   ./shuffle_geom_check                                    the built-in shape list
//   ./shuffle_geom_check NPIX/Cpad_in,c_off,C,groups ...    these cases instead; tests pass the GPU tests' list
// One line per case: "case NPIX/Cpad_in,c_off,C,g: lds L tile TP tiles T blocks B", then "ok, <bytes> bytes checked".  Exit
// status 1 at the first violation.
// The walk below is the kernel's own: the same launch size, the same tile -> workgroup stride loop, the same stage items and
// byte walk (shuf_* of the header), on a model of memory whose every byte is its own address, so that a wrong byte is seen as
// well as a wrong address.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_shuffle_i8_geom.h"

using namespace fq;

struct Case { long npix; int Cpad_in, c_off, C, g; std::string text; };

static void fail(const char* what, const Case& c) {
    printf("%s: %s\n", what, c.text.c_str());
    exit(1);
}

static long run(const Case& c, bool print) {
    if (!shuf_args_ok(c.Cpad_in, c.c_off, c.C, c.g)) fail("arguments the entry point refuses", c);
    if (c.npix < 1 || c.npix * c.Cpad_in >= 0x7fffffffL || c.npix * shuf_pad16(c.C) >= 0x7fffffffL) fail("size the entry point refuses", c);
    const ShufGeom s = shuf_geom(c.Cpad_in, c.c_off, c.C, c.g, (unsigned)c.npix);
    const long src_bytes = c.npix * s.Cpad_in, out_bytes = c.npix * s.Cpad_out;
    const unsigned blocks = shuf_blocks(s);
    if (print) printf("case %s: lds %d tile %d tiles %u blocks %u\n", c.text.c_str(), s.lds, s.TP, s.ntiles, blocks);
    if (s.TP < 1 || s.S % 16 || s.a0 % 16 || s.a0 < 0 || s.a0 + s.S > s.Cpad_in || s.a0 > s.c_off || s.c_off + s.C > s.a0 + s.S)
        fail("span is not an aligned part of the row that holds the channels", c);
    if (s.lds && (long)s.TP * s.S > kShufLdsBytes) fail("tile does not fit the LDS", c);
    if ((unsigned long)s.ntiles * s.TP < (unsigned long)c.npix || (unsigned long)(s.ntiles - 1) * s.TP >= (unsigned long)c.npix)
        fail("tiles do not cover the pixels", c);
    if ((unsigned long)s.ntiles * s.TP + blocks > 0xffffffffUL) fail("32-bit tile arithmetic wraps", c);
    std::vector<unsigned char> written((size_t)out_bytes, 0);
    std::vector<long> lds(s.lds ? kShufLdsBytes : 0);
    long checked = 0;
    for (unsigned b = 0; b < blocks; ++b) {
        for (unsigned t = b; t < s.ntiles; t += blocks) {
            const unsigned pix0 = t * (unsigned)s.TP, np = shuf_tile_pixels(s, t);
            if (np < 1 || np > (unsigned)s.TP || (long)pix0 + np > c.npix) fail("tile reaches past the last pixel", c);
            long staged = 0;
            if (s.lds) {
                const unsigned items = np * (unsigned)s.SU;
                for (unsigned tid = 0; tid < (unsigned)kShufBlock; ++tid)
                    for (unsigned i = tid; i < items; i += kShufBlock) {
                        const size_t o = shuf_stage_src(s, pix0, i);
                        if (o % 16 || (long)o + 16 > src_bytes) fail("stage load outside the source or unaligned", c);
                        if (16l * i + 16 > kShufLdsBytes) fail("stage store outside the LDS", c);
                        for (int k = 0; k < 16; ++k) lds[16 * (size_t)i + k] = (long)o + k;
                    }
                staged = 16l * items;
            }
            const unsigned units = np * (unsigned)s.CH;
            for (unsigned tid = 0; tid < (unsigned)kShufBlock; ++tid)
                for (unsigned o = tid; o < units; o += kShufBlock) {
                    const unsigned p = o / (unsigned)s.CH, k = o - p * (unsigned)s.CH;
                    const size_t base = shuf_row_base(s, pix0, p);
                    ShufWalk w = shuf_walk_begin(s, k);
                    const long pix = (long)pix0 + p;
                    const long store = pix * s.Cpad_out + 16l * k;
                    if (store % 16 || store + 16 > out_bytes) fail("store outside the output or unaligned", c);
                    for (int byte = 0; byte < 16; ++byte) {
                        const long j = 16l * k + byte;
                        if ((long)w.j != j) fail("the walk lost its channel", c);
                        long got = -1;
                        if (shuf_walk_real(s, w)) {
                            const long a = (long)base + shuf_walk_rel(s, w);
                            if (s.lds) {
                                if (a < 0 || a >= staged) fail("LDS read outside what the tile staged", c);
                                got = lds[(size_t)a];
                            } else {
                                if (a < 0 || a >= src_bytes) fail("byte load outside the source", c);
                                got = a;
                            }
                        }
                        const long want = j < c.C ? pix * s.Cpad_in + c.c_off + (j % c.g) * (long)(c.C / c.g) + j / c.g : -1;
                        if (got != want) fail("output byte is not the byte the index rule names", c);
                        if (want >= 0 && (want < pix * s.Cpad_in + c.c_off || want >= pix * s.Cpad_in + c.c_off + c.C))
                            fail("the rule itself leaves the channel range", c);
                        if (written[(size_t)store + byte]++) fail("output byte written twice", c);
                        shuf_walk_next(s, w);
                        ++checked;
                    }
                }
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output byte not written", c);
    return checked;
}

static Case make(long npix, int Cpad_in, int c_off, int C, int g) {
    Case c;
    c.npix = npix; c.Cpad_in = Cpad_in; c.c_off = c_off; c.C = C; c.g = g;
    c.text = std::to_string(npix) + "/" + std::to_string(Cpad_in) + "," + std::to_string(c_off) + "," + std::to_string(C) + "," + std::to_string(g);
    return c;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        long npix;
        int cp, off, C, g;
        if (sscanf(argv[a], "%ld/%d,%d,%d,%d", &npix, &cp, &off, &C, &g) != 5) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(make(npix, cp, off, C, g));
    }
    if (cases.empty()) {
        const int shuffles[][2] = {{8, 2}, {20, 2}, {116, 2}, {12, 3}, {60, 3}, {240, 3}, {16, 4}, {96, 8}, {24, 8}, {6, 6}, {244, 2},
                                   {7, 7}, {1, 1}, {976, 2}, {48, 4}, {30, 5}};
        const int slices[][3] = {{128, 58, 58}, {32, 10, 10}, {32, 0, 10}, {256, 122, 122}, {16, 15, 1}, {64, 16, 48}, {64, 63, 1},
                                 {48, 1, 47}, {496, 244, 244}};
        const long pixels[] = {1, 3, kShufTilePix - 1, kShufTilePix, kShufTilePix + 1, 2 * 7 * 9, 1000};
        for (long px : pixels) {
            for (const auto& sh : shuffles)
                if (sh[1] != 1) cases.push_back(make(px, shuf_pad16(sh[0]), 0, sh[0], sh[1]));    // (one group, no offset: nothing to do)
            for (const auto& sl : slices) cases.push_back(make(px, sl[0], sl[1], sl[2], 1));
            cases.push_back(make(px, 64, 5, 18, 3));                       // both at once
            cases.push_back(make(px, 64, 5, 18, 18));
        }
        cases.push_back(make((long)kShufMaxBlocks * kShufTilePix + 1, 16, 0, 8, 2));     // one tile more than workgroups: the stride loop
        cases.push_back(make((long)kShufMaxBlocks * kShufTilePix * 2 + 70, 32, 3, 20, 4));
        cases.push_back(make(70, 1024, 500, 510, 2));                      // a span that shortens the tile (TP < kShufTilePix)
        cases.push_back(make(5, 16384, 100, 16000, 4));                    // ... to two pixels
        cases.push_back(make(3, 32768, 0, 32768, 2));                      // ... to one
        cases.push_back(make(3, 32784, 1, 32768, 2));                      // a span above the LDS budget: read from global memory
        cases.push_back(make(2, 65552, 7, 65536, 8));                      // the widest row the entry point takes
    }
    long total = 0;
    for (const Case& c : cases) total += run(c, argc > 1);
    printf("ok, %ld bytes checked\n", total);
    return 0;
}
