// act_lut_geom_check.cpp -- the index arithmetic of fq_act_lut_i8_nhwc (csrc/fq_act_lut_i8_geom.h) walked on the host.
//
//   g++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o act_lut_geom_check scripts/act_lut_geom_check.cpp
//   ./act_lut_geom_check N,H,W,C,Cpad [N,H,W,C,Cpad ...]
//
// For every case the kernel's loop is replayed lane by lane: every workgroup of the grid, every lane, every pass of the chunk loop,
// then the tail bytes of workgroup 0, on real buffers of exactly N*H*W*Cpad bytes (so the address sanitizer sees any access
// outside them) and a table of exactly 256 bytes.  Checked: each output byte is written exactly once; a real channel holds
// table[x + 128] and a padding channel zero though the table holds 77 at index 128; no index leaves x, y or the table.
// Prints one line per case ("case N,H,W,C,Cpad: chunks .. tail .. blocks .. passes ..") and "ok, <cases> cases" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_act_lut_i8_geom.h"

using namespace fq;

static int fail(const char* what, const char* arg, unsigned long long at) {
    std::printf("FAILED case %s: %s at %llu\n", arg, what, at);
    return 1;
}

static int run(const char* arg) {
    int N, H, W, C, Cpad;
    if (std::sscanf(arg, "%d,%d,%d,%d,%d", &N, &H, &W, &C, &Cpad) != 5) return fail("cannot parse", arg, 0);
    if (act_lut_args(N, H, W, C, Cpad) != 0) return fail("refused by act_lut_args", arg, 0);
    const ActLutGeom g = act_lut_geom((unsigned)((long)N * H * W), C, Cpad);
    const size_t n = (size_t)N * H * W * Cpad;
    if (g.n != n || (size_t)g.chunks * 16 + g.tail != n || g.blocks < 1 || g.blocks > (unsigned)kActLutMaxBlocks)
        return fail("geometry", arg, g.n);
    std::vector<int8_t> x(n), y(n, 0), table(256);
    std::vector<unsigned char> written(n, 0);
    for (size_t i = 0; i < n; ++i) x[i] = (int8_t)((i * 37u + (i >> 8)) & 0xff);
    for (int i = 0; i < 256; ++i) table[i] = (int8_t)((i * 91 + 5) & 0xff);
    table[128] = 77;
    for (unsigned block = 0; block < g.blocks; ++block)
        for (unsigned tid = 0; tid < (unsigned)kActLutBlock; ++tid) {
            for (unsigned p = 0; p < g.passes; ++p) {
                const unsigned long long chunk = act_lut_chunk(g, block, tid, p);
                if (chunk >= g.chunks) continue;
                const unsigned o = (unsigned)chunk * 16u;
                const unsigned m = act_lut_real_mask(g, o);
                for (unsigned k = 0; k < 16; ++k) {
                    const size_t at = (size_t)o + k;
                    if (at >= n) return fail("chunk byte outside the tensor", arg, at);
                    const unsigned bits4 = (m >> (4 * (k / 4))) & 15u;
                    const unsigned keep = (act_lut_byte_mask(bits4) >> (8 * (k % 4))) & 0xffu;
                    const unsigned idx = (unsigned)(x.at(at) + 128);
                    y.at(at) = (int8_t)((unsigned char)table.at(idx) & keep);
                    if (written[at]++) return fail("output byte written twice", arg, at);
                }
            }
            if (block == 0 && tid < g.tail) {
                const size_t at = act_lut_tail_offset(g, tid);
                if (at >= n) return fail("tail byte outside the tensor", arg, at);
                y.at(at) = act_lut_tail_real(g, tid) ? table.at((unsigned)(x.at(at) + 128)) : (int8_t)0;
                if (written[at]++) return fail("output byte written twice", arg, at);
            }
        }
    for (size_t at = 0; at < n; ++at) {
        if (written[at] != 1) return fail("output byte not written", arg, at);
        const int8_t want = (int)(at % (size_t)Cpad) < C ? table[(unsigned)(x[at] + 128)] : (int8_t)0;
        if (y[at] != want) return fail("wrong byte", arg, at);
    }
    std::printf("case %s: chunks %u tail %u blocks %u passes %u\n", arg, g.chunks, g.tail, g.blocks, g.passes);
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (run(argv[i])) return 1;
    std::printf("ok, %d cases\n", argc - 1);
    return 0;
}
