// Host emulation of gconv_i8_kernel (csrc/fq_gconv_i8.hip): the kernel's loops written out in C++ over the same geometry functions
// (csrc/fq_gconv_i8_geom.h) -- staging into an LDS array, lanes, strips, chunks, taps, dot4, the four-instruction tail -- against a
// direct grouped convolution with the reference's tail, over the GPU tests' widths, kernels, strides, paddings, planes and batches.
//   c++ -O2 -std=c++17 -o gconv_emul_check scripts/gconv_emul_check.cpp && ./gconv_emul_check
// (tests/test_grouped_plan_cpu.py runs it.)  It says nothing about the compiled kernel; it says that the decomposition, the packed
// layout and the index functions compute the convolution of include/fq.h, padding channels and image borders included.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include <random>
#include "../pytorch-quantity_amd/csrc/fq_gconv_i8_geom.h"
using namespace fq;
static int dot4(unsigned a, unsigned b, int c) { for (int i = 0; i < 4; ++i) c += (int)(int8_t)(a >> (8*i)) * (int)(int8_t)(b >> (8*i)); return c; }
static int med3(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int tail_ref(int acc, int qb, int rs, bool relu) { // RightShift round half away, clamp, + bias, clamp
    long a = acc; long r = (a + (1L << (rs-1)) + (a < 0 ? -1 : 0)) >> rs; r = r < -128 ? -128 : (r > 127 ? 127 : r);
    r += qb; long lo = relu ? 0 : -128; return (int)(r < lo ? lo : (r > 127 ? 127 : r)); }
int run(int G, int cgi, int cgo, int R, int ST, int pad, int N, int H, int W, int rs, bool relu, unsigned seed) {
    int C = G*cgi, K = G*cgo; GcGeom g; if (H+2*pad<R||W+2*pad<R) return 0;
    gc_setup(g, N, H, W, C, K, G, R, ST, pad, pad);
    std::mt19937 rng(seed);
    std::vector<int8_t> x((size_t)N*H*W*g.Cpad), w((size_t)K*cgi*R*R), pk((size_t)g.Kpad*R*R*cgi, 0), q((size_t)N*g.P*g.Q*g.Kpad, 77);
    for (auto& v : x) v = (int8_t)(rng()%256-128); for (auto& v : w) v = (int8_t)(rng()%256-128);
    std::vector<int> qb(K); for (auto& v : qb) v = (int)(rng()%300) - 150;
    for (int k = 0; k < K; ++k) for (int j = 0; j < cgi; ++j) for (int t = 0; t < R*R; ++t)
        pk[(((size_t)(k/4)*R*R + t)*(cgi/4) + j/4)*16 + 4*(k%4) + j%4] = w[((size_t)k*cgi + j)*R*R + t];
    unsigned blocks = gc_blocks(g), step = gc_sb_step(g, blocks);
    std::vector<unsigned> lds((size_t)g.units*4);
    const int TQ = kGcTQ, NPIX = (TQ-1)*ST + R;
    for (unsigned b = 0; b < blocks; ++b) {
        int kb = gc_block_kb(g, b);
        for (unsigned i = 0; i < g.units; ++i) for (int d = 0; d < 4; ++d) lds[gc_stage_dst(g,i)*4+d] = ((unsigned*)pk.data())[gc_stage_src(g,kb,i)*4+d];
        for (int lane = 0; lane < kGcBlock; ++lane) {
            int kql = gc_lane_quad(g, lane), ls = gc_lane_strip(g, lane), kq = gc_quad(g, kb, kql); bool valid = gc_quad_valid(g, kq);
            for (unsigned sb = gc_block_sb0(g, b); sb < g.sblocks; sb += step) {
                unsigned strip = sb*g.SPW + ls; if (strip >= g.strips) continue;
                GcStripPos sp = gc_strip_pos(g, strip);
                int ih0 = sp.p*ST - g.pad_h, iw0 = sp.q0*ST - g.pad_w; int acc[4][4] = {};
                if (valid) for (int j4 = 0; j4 < g.CH; ++j4) { int chan = gc_in_chan(g, kq, j4);
                    for (int r = 0; r < R; ++r) { int ih = ih0 + r; unsigned xv[16];
                        for (int k = 0; k < NPIX; ++k) { xv[k] = 0; if (gc_in_ok(g, ih, iw0+k)) xv[k] = *(unsigned*)(x.data() + gc_in_off(g, sp.n, ih, iw0+k, chan)); }
                        for (int s = 0; s < R; ++s) { const unsigned* wv = &lds[gc_lds_unit(g, kql, r*R+s, j4)*4];
                            for (int j = 0; j < TQ; ++j) for (int c = 0; c < 4; ++c) acc[c][j] = dot4(xv[j*ST+s], wv[c], acc[c][j]); } } }
                for (int j = 0; j < TQ; ++j) { if (!gc_out_ok(g, sp.q0+j)) continue;
                    for (int c = 0; c < 4; ++c) { int ch = 4*kq+c; int v = 0;
                        if (valid) { int qbc = med3(qb[ch], (relu?0:-128)-127, 127+128); int B = (1<<(rs-1)) + (qbc<<rs);
                            int lo = med3(-128+qbc, relu?0:-128, 127), hi = med3(127+qbc, relu?0:-128, 127);
                            v = med3((acc[c][j] + B + (acc[c][j]>>31)) >> rs, lo, hi); }
                        q[gc_out_off(g, sp.n, sp.p, sp.q0+j, kq) + c] = (int8_t)v; } }
            }
        }
    }
    for (int n = 0; n < N; ++n) for (int p = 0; p < g.P; ++p) for (int qq = 0; qq < g.Q; ++qq) for (int k = 0; k < g.Kpad; ++k) {
        int want = 0;
        if (k < K) { int acc = 0; for (int r = 0; r < R; ++r) for (int s = 0; s < R; ++s) { int ih = p*ST-pad+r, iw = qq*ST-pad+s; if (ih<0||ih>=H||iw<0||iw>=W) continue;
            for (int j = 0; j < cgi; ++j) acc += (int)w[((size_t)k*cgi+j)*R*R + r*R+s] * (int)x[(((size_t)n*H+ih)*W+iw)*g.Cpad + (k/cgo)*cgi + j]; }
            want = tail_ref(acc, qb[k], rs, relu); }
        int got = q[(((size_t)n*g.P+p)*g.Q+qq)*g.Kpad + k];
        if (got != want) { printf("MISMATCH G%d cgi%d cgo%d R%d s%d p%d N%d %dx%d n%d p%d q%d k%d got %d want %d\n", G,cgi,cgo,R,ST,pad,N,H,W,n,p,qq,k,got,want); exit(1); } }
    return 1;
}
int main() { int widths[][3] = {{2,4,4},{8,4,4},{3,8,4},{2,16,8},{2,32,32},{2,64,64},{5,4,12},{32,4,4}}; int planes[][2] = {{1,1},{2,2},{5,7},{9,11},{33,17}}; int n = 0, i = 0;
    for (auto& wd : widths) for (int R : {1,3}) for (int st : {1,2}) for (int pad = 0; pad < R; ++pad) for (auto& hw : planes) for (int N : {1,3}) { int rs = (int[]){1,7,16}[i%3]; n += run(wd[0],wd[1],wd[2],R,st,pad,N,hw[0],hw[1],rs,(i/3)%2,i); ++i; }
    printf("ok %d cases\n", n); }
