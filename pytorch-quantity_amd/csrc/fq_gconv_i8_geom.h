// fq_gconv_i8_geom.h -- the workgroup / lane -> tile, address, tap, LDS index and channel mask arithmetic of the grouped int8
// convolution (fq_gconv_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/gconv_geom_check.cpp walks them over the shapes the GPU tests run and asserts that every address a lane may touch lies
// inside its tensor, every tap reads the pixel and channel the rule names, and every output dword is written exactly once.
#pragma once

#if defined(__HIPCC__)
#define FQ_GC_HD __host__ __device__ __forceinline__
#else
#define FQ_GC_HD inline
#endif

namespace fq {

constexpr int kGcBlock = 256;          // threads per workgroup
constexpr int kGcTQ = 4;               // output columns per lane: a strip of one output row
constexpr int kGcMaxBlocks = 2048;     // 256 CUs x 8 workgroups: the workgroups walk the rest of the tiles
constexpr int kGcUnit = 16;            // bytes of one weight unit: 4 output channels x 4 input channels of one tap

struct GcGeom {
    int N, H, W, P, Q;
    int C, K, Cpad, Kpad;
    int Cgi, Cgo;                      // input / output channels per group
    int CH;                            // Cgi / 4: 4-channel chunks of a group's input
    int RS;                            // taps
    int S;                             // kernel width (= height)
    int stride, pad_h, pad_w;
    int KB4;                           // output-channel quads per workgroup: 16, 8 or 4 (64 / 32 / 16 channels)
    int KBn;                           // channel blocks: Kpad / (4 * KB4)
    int SPW;                           // strips per workgroup step: kGcBlock / KB4
    int QS;                            // strips per output row: ceil(Q / kGcTQ)
    unsigned strips;                   // N * P * QS
    unsigned sblocks;                  // ceil(strips / SPW)
    unsigned units;                    // weight units of one channel block: KB4 * RS * CH (staged in LDS)
};

// Fills every derived field from the layer.  false: the launch does not fit (more channel blocks than workgroups).
FQ_GC_HD bool gc_setup(GcGeom& g, int N, int H, int W, int C, int K, int groups, int R, int stride, int pad_h, int pad_w) {
    g.N = N; g.H = H; g.W = W; g.C = C; g.K = K;
    g.Cpad = (C + 15) / 16 * 16; g.Kpad = (K + 15) / 16 * 16;
    g.Cgi = C / groups; g.Cgo = K / groups; g.CH = g.Cgi / 4;
    g.RS = R * R; g.S = R; g.stride = stride; g.pad_h = pad_h; g.pad_w = pad_w;
    g.P = (H + 2 * pad_h - R) / stride + 1;
    g.Q = (W + 2 * pad_w - R) / stride + 1;
    const int kb = g.Kpad % 64 == 0 ? 64 : (g.Kpad % 32 == 0 ? 32 : 16);
    g.KB4 = kb / 4; g.KBn = g.Kpad / kb; g.SPW = kGcBlock / g.KB4;
    g.QS = (g.Q + kGcTQ - 1) / kGcTQ;
    g.strips = (unsigned)N * g.P * g.QS;
    g.sblocks = (g.strips + g.SPW - 1) / g.SPW;
    g.units = (unsigned)g.KB4 * g.RS * g.CH;
    return g.KBn <= kGcMaxBlocks;
}

// workgroups of the launch: a multiple of KBn, so that workgroup b keeps channel block b % KBn while it steps over strip blocks
FQ_GC_HD unsigned gc_blocks(const GcGeom& g) {
    unsigned per = (unsigned)(kGcMaxBlocks / g.KBn);
    if (per > g.sblocks) per = g.sblocks;
    return per * (unsigned)g.KBn;
}
FQ_GC_HD int gc_block_kb(const GcGeom& g, unsigned block) { return (int)(block % (unsigned)g.KBn); }
FQ_GC_HD unsigned gc_block_sb0(const GcGeom& g, unsigned block) { return block / (unsigned)g.KBn; }
FQ_GC_HD unsigned gc_sb_step(const GcGeom& g, unsigned blocks) { return blocks / (unsigned)g.KBn; }

// lane -> (channel quad of the block, strip of the step): neighbouring lanes are neighbouring quads of the same pixels
FQ_GC_HD int gc_lane_quad(const GcGeom& g, int lane) { return lane % g.KB4; }
FQ_GC_HD int gc_lane_strip(const GcGeom& g, int lane) { return lane / g.KB4; }
FQ_GC_HD int gc_quad(const GcGeom& g, int kb, int kql) { return kb * g.KB4 + kql; }       // output channels 4 * quad .. + 3
// the channel mask: quads at or beyond K are padding -- they read nothing and write zeros
FQ_GC_HD bool gc_quad_valid(const GcGeom& g, int kq) { return 4 * kq < g.K; }

struct GcStripPos { int n, p, q0; };
FQ_GC_HD GcStripPos gc_strip_pos(const GcGeom& g, unsigned strip) {
    GcStripPos t;
    const unsigned qs = strip % (unsigned)g.QS, rest = strip / (unsigned)g.QS;
    t.q0 = (int)qs * kGcTQ;
    t.p = (int)(rest % (unsigned)g.P);
    t.n = (int)(rest / (unsigned)g.P);
    return t;
}

// first input channel of chunk j4 of the group that output quad kq belongs to (a valid quad only)
FQ_GC_HD int gc_in_chan(const GcGeom& g, int kq, int j4) { return (4 * kq / g.Cgo) * g.Cgi + 4 * j4; }
FQ_GC_HD bool gc_in_ok(const GcGeom& g, int ih, int iw) { return (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W; }
FQ_GC_HD unsigned gc_in_off(const GcGeom& g, int n, int ih, int iw, int chan) {
    return (((unsigned)n * g.H + ih) * g.W + iw) * g.Cpad + (unsigned)chan;
}
FQ_GC_HD bool gc_out_ok(const GcGeom& g, int q) { return q < g.Q; }
FQ_GC_HD unsigned gc_out_off(const GcGeom& g, int n, int p, int q, int kq) {
    return (((unsigned)n * g.P + p) * g.Q + q) * g.Kpad + 4u * kq;
}

// packed weights (include/fq.h): unit ((kq * RS + t) * CH + j4), 16 bytes each; a channel block is `units` consecutive units
FQ_GC_HD unsigned gc_w_unit(const GcGeom& g, int kq, int t, int j4) { return ((unsigned)kq * g.RS + t) * g.CH + j4; }
FQ_GC_HD unsigned gc_stage_src(const GcGeom& g, int kb, unsigned i) { return (unsigned)kb * g.units + i; }
// LDS: quads innermost, so the lanes of a wave read consecutive 16-byte units (no bank conflict)
FQ_GC_HD unsigned gc_lds_unit(const GcGeom& g, int kql, int t, int j4) { return ((unsigned)t * g.CH + j4) * g.KB4 + kql; }
// unit i of the block in global order (kql, t, j4) -> its LDS slot
FQ_GC_HD unsigned gc_stage_dst(const GcGeom& g, unsigned i) {
    const unsigned per = (unsigned)g.RS * g.CH;
    return (i % per) * g.KB4 + i / per;
}

}  // namespace fq
