// fq_add_up.hip -- the resident NewAdd whose second operand is read through a nearest upsampling by 2 or 4 (include/fq.h:
// fq_add_up_resident).  The FPN top-down step Eltwise(lateral, up(top)): `top` is an int8 activation or the exact int16 sum of the
// NewAdd one level up, and the s*s times larger upsampled tensor is neither written nor read back.
//
// The rule is fq_add_resident's, word for word, on (x[n, h, w, c], y[n, h / up, w / up, c]): nearest upsampling repeats values,
// so the parameters are make_add_params' and the arithmetic is add_resident_16 (fq_resident.h) -- the packed int16, int32 or fp32
// form, chosen uniformly per launch as there.  Nothing of either is copied here.
// A bandwidth kernel without LDS, shaped like add_resident_kernel:
//   * one item is 16 channels of one output pixel (fq_add_up_geom.h): a 16-byte load per int8 operand, two per int16 operand, one
//     16-byte store for the int8 re-quantisation and two for the exact sum -- plain stores, which keep the lines in the L2 for
//     the convolution behind the add;
//   * consecutive lanes walk the channels of a pixel, then the pixels of a row, so a wave reads and writes contiguous bytes of
//     x and the outputs, and the `up` neighbouring pixels that share a coarse pixel read the same lines of y (each coarse row
//     is read by `up` output rows: the re-reads hit the L2, HBM sees y once);
//   * at most 4096 workgroups of 256 lanes (res_grid's cap); a lane's first item is split into (n, h, w, k) by division, every
//     further one by adding the split of the stride digit by digit (add_up_next): no division inside the loop.
// Every access is 16-byte aligned and lies inside its tensor; scripts/add_up_geom_check.cpp walks the same functions on the host.
#include "fq_resident.h"
#include "fq_add_up_geom.h"

namespace fq {

template <typename TX, typename TY>
__global__ __launch_bounds__(kAddUpBlock) void add_up_resident_kernel(const TX* __restrict__ x, const TY* __restrict__ y,
                                                                     int16_t* __restrict__ wide, int8_t* __restrict__ narrow,
                                                                     const AddUpGeom g, const AddResParams p) {
    size_t i = (size_t)blockIdx.x * kAddUpBlock + threadIdx.x;
    if (i >= g.items) return;
    const size_t stride = (size_t)gridDim.x * kAddUpBlock;
    AddUpItem c = add_up_first(g, i);
    for (;;) {
        Vec16<TX> vx; Vec16<TY> vy;
        vx.load(x + i * 16);
        vy.load(y + add_up_coarse(g, c) * 16);
        add_resident_16(vx, vy, wide ? wide + i * 16 : nullptr, narrow ? narrow + i * 16 : nullptr, p);
        i += stride;
        if (i >= g.items) break;
        c = add_up_next(g, c);
    }
}

template <typename TX, typename TY>
static void launch_add_up(hipStream_t st, const void* x, const void* y, int16_t* wide, int8_t* narrow, const AddUpGeom& g,
                          const AddResParams& p) {
    hipLaunchKernelGGL((add_up_resident_kernel<TX, TY>), dim3(add_up_blocks(g.items)), dim3(kAddUpBlock), 0, st,
                       static_cast<const TX*>(x), static_cast<const TY*>(y), wide, narrow, g, p);
}

static bool add_up_supported(int up, int H, int W, int Cpad) {
    if (add_up_log2(up) < 0 || H <= 0 || W <= 0 || Cpad <= 0 || (Cpad & 15)) return false;
    return H % up == 0 && W % up == 0;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_add_up_resident_supported(int up, int H, int W, int Cpad) { return add_up_supported(up, H, W, Cpad) ? 1 : 0; }

extern "C" int fq_add_up_resident(const void* x, int x_bytes, int gx, const void* y, int y_bytes, int gy, int up, int16_t* wide,
                                  int g_wide, int8_t* narrow, int ib, int relu, int N, int H, int W, int Cpad, fq_stream_t stream) {
    if ((x_bytes != 1 && x_bytes != 2) || (y_bytes != 1 && y_bytes != 2)) return FQ_ERR_INVALID_ARG;
    if (N < 0 || H < 0 || W < 0 || Cpad < 0 || (Cpad & 15)) return FQ_ERR_INVALID_ARG;       // NHWC rows are padded to 16 channels
    if (up != 2 && up != 4) return FQ_ERR_UNSUPPORTED;
    if (N == 0 || H == 0 || W == 0 || Cpad == 0) return FQ_OK;
    if (H % up || W % up) return FQ_ERR_INVALID_ARG;
    if (!x || !y || (!wide && !narrow)) return FQ_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(wide) |
         reinterpret_cast<uintptr_t>(narrow)) & 15u)
        return FQ_ERR_INVALID_ARG;
    AddResParams p;
    const int rc = make_add_params(gx, gy, g_wide, wide != nullptr, ib, relu, &p);
    if (rc != FQ_OK) return rc;
    const AddUpGeom g = add_up_geom(N, H, W, Cpad, up);
    hipStream_t st = as_stream(stream);
    if (x_bytes == 1 && y_bytes == 1) launch_add_up<int8_t, int8_t>(st, x, y, wide, narrow, g, p);
    else if (x_bytes == 1) launch_add_up<int8_t, int16_t>(st, x, y, wide, narrow, g, p);
    else if (y_bytes == 1) launch_add_up<int16_t, int8_t>(st, x, y, wide, narrow, g, p);
    else launch_add_up<int16_t, int16_t>(st, x, y, wide, narrow, g, p);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
