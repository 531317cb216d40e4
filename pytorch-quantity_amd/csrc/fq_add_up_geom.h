// fq_add_up_geom.h -- the lane -> (output item, operand offsets) arithmetic of the resident NewAdd whose second operand is read
// through a nearest upsampling (fq_add_up.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/add_up_geom_check.cpp walks them over the shapes the GPU tests and the FPN model run and asserts that every load lies
// inside its source, that every access is 16-byte aligned, that the coarse pixel is (h / up, w / up) and that every output element
// is written exactly once.
//
// x and the outputs are [N][H][W][Cpad], y is [N][H / up][W / up][Cpad]; up is 2 or 4 (lg = 1 or 2), H and W are multiples of it.
// An ITEM is 16 consecutive channels of one output pixel, CH = Cpad / 16 items per pixel, item i = ((n H + h) W + w) CH + k:
// channel fastest, then w -- so the lanes of a wave walk whole pixels of one row, and the `up` neighbouring pixels that share a
// coarse pixel read the same lines of y.  Offsets are in ITEMS of the flat tensors (size_t): an operand's byte offset is
// 16 * element size * its item offset, every access a multiple of 16 bytes.
//
// The lane -> item map.  A launch has B = add_up_blocks(items) workgroups of kAddUpBlock lanes; lane t (global index) takes the
// items t, t + S, t + 2 S, ... with S = B kAddUpBlock.  Only the FIRST item of a lane is split into (n, h, w, k) by division
// (add_up_first); every further one is reached by adding the split of S digit by digit with at most one carry per digit
// (add_up_next), so the loop has no division by a run-time value.  The coarse item of (n, h, w, k) is shifts and multiplications.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define FQ_ADDUP_HD __host__ __device__ __forceinline__
#else
#define FQ_ADDUP_HD inline
#endif

namespace fq {

constexpr int kAddUpBlock = 256;                 // threads per workgroup
constexpr int kAddUpMaxBlocks = 256 * 16;        // res_grid's cap (fq_resident.hip): 16 workgroups for each of the 256 CUs

struct AddUpItem { int n, h, w, k; };

struct AddUpGeom {
    int N, H, W, CH;                   // output plane, CH = Cpad / 16
    int Hc, Wc, lg;                    // coarse plane H >> lg, W >> lg; lg = log2(up)
    size_t items;                      // N H W CH
    AddUpItem step;                    // the launch's stride S split as (S / (H W CH), S / (W CH) % H, S / CH % W, S % CH)
};

FQ_ADDUP_HD int add_up_log2(int up) { return up == 2 ? 1 : (up == 4 ? 2 : -1); }

// workgroups of one launch: one lane per item up to the cap, at least one
FQ_ADDUP_HD unsigned add_up_blocks(size_t items) {
    size_t b = (items + kAddUpBlock - 1) / kAddUpBlock;
    if (b > (size_t)kAddUpMaxBlocks) b = (size_t)kAddUpMaxBlocks;
    return (unsigned)(b ? b : 1);
}

// item i split into its digits (division: once per lane, and once per launch for the stride)
FQ_ADDUP_HD AddUpItem add_up_split(int H, int W, int CH, size_t i) {
    AddUpItem c;
    c.k = (int)(i % (size_t)CH);
    size_t r = i / (size_t)CH;
    c.w = (int)(r % (size_t)W);
    r /= (size_t)W;
    c.h = (int)(r % (size_t)H);
    c.n = (int)(r / (size_t)H);
    return c;
}

FQ_ADDUP_HD AddUpGeom add_up_geom(int N, int H, int W, int Cpad, int up) {
    AddUpGeom g;
    g.N = N; g.H = H; g.W = W; g.CH = Cpad / 16;
    g.lg = add_up_log2(up);
    g.Hc = H >> g.lg; g.Wc = W >> g.lg;
    g.items = (size_t)N * (size_t)H * (size_t)W * (size_t)g.CH;
    g.step = add_up_split(H, W, g.CH, (size_t)add_up_blocks(g.items) * kAddUpBlock);
    return g;
}

FQ_ADDUP_HD AddUpItem add_up_first(const AddUpGeom& g, size_t i) { return add_up_split(g.H, g.W, g.CH, i); }

// the item S further on: digit-wise addition, every digit of both summands is below its base, so one carry at most
FQ_ADDUP_HD AddUpItem add_up_next(const AddUpGeom& g, AddUpItem c) {
    c.k += g.step.k;
    int carry = c.k >= g.CH;
    c.k -= carry ? g.CH : 0;
    c.w += g.step.w + carry;
    carry = c.w >= g.W;
    c.w -= carry ? g.W : 0;
    c.h += g.step.h + carry;
    carry = c.h >= g.H;
    c.h -= carry ? g.H : 0;
    c.n += g.step.n + carry;
    return c;
}

// offset, in items, of (n, h, w, k) in x and in the outputs
FQ_ADDUP_HD size_t add_up_fine(const AddUpGeom& g, const AddUpItem& c) {
    return (((size_t)c.n * (size_t)g.H + (size_t)c.h) * (size_t)g.W + (size_t)c.w) * (size_t)g.CH + (size_t)c.k;
}

// offset, in items, of the coarse pixel (n, h / up, w / up) at the same channels in y
FQ_ADDUP_HD size_t add_up_coarse(const AddUpGeom& g, const AddUpItem& c) {
    return (((size_t)c.n * (size_t)g.Hc + (size_t)(c.h >> g.lg)) * (size_t)g.Wc + (size_t)(c.w >> g.lg)) * (size_t)g.CH + (size_t)c.k;
}

}  // namespace fq
