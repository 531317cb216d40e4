// Timing probe only, never loaded by the product (scripts/avgpool_i16_lane_probe.py): the 16-channels-per-lane form of the average
// pool over an int16 sum, to set against the library's 8-channel form (csrc/fq_avgpool_i16.hip).  Two 16-byte
// loads per tap, sixteen int32 accumulators and divisions per lane, one 16-byte store.  Same rule, same launch shape; the int8
// pool's geometry header serves as it stands (a chunk of 16 channels is 32 source bytes: byte offsets are twice its offsets).
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -shared -o scripts/_bin/libavg16c.so scripts/avgpool_i16_c16_probe.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../pytorch-quantity_amd/csrc/fq_avgpool_i8_geom.h"
using namespace fq;
struct P16 { AvgGeom g; float scale, lo; };
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned rq(int s, float d, float scale, float lo) {
    const float r = rintf(((float)s / d) * scale);
    return (unsigned)(int)fminf(fmaxf(r, lo), 127.0f) & 0xffu;
}
__global__ __launch_bounds__(kAvgBlock) void avgpool_i16_c16_kernel(const int16_t* __restrict__ x, int8_t* __restrict__ y, const P16 p) {
    const AvgGeom& g = p.g;
    const unsigned stride = gridDim.x * kAvgBlock;
    const unsigned step = 2u * (unsigned)g.Cpad;
    const char* xb = reinterpret_cast<const char*>(x);
    for (unsigned i = blockIdx.x * kAvgBlock + threadIdx.x; i < g.nchunks; i += stride) {
        const AvgChunk c = avg_chunk(g, i);
        const AvgWindow w = avg_window(g, c.p, c.q);
        int s[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = 0;
        for (int ih = w.h0; ih < w.h1; ++ih) {
            unsigned off = 2u * avg_tap_offset(g, c.n, ih, w.w0, c.k);
            for (int iw = w.w0; iw < w.w1; ++iw, off += step) {
                const v4u a = *reinterpret_cast<const v4u*>(xb + off);
                const v4u b = *reinterpret_cast<const v4u*>(xb + off + 16);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s[2 * t] += (int)(a[t] << 16) >> 16;  s[2 * t + 1] += (int)a[t] >> 16;
                    s[8 + 2 * t] += (int)(b[t] << 16) >> 16;  s[8 + 2 * t + 1] += (int)b[t] >> 16;
                }
            }
        }
        const float div = (float)avg_divisor(g, w);
        v4u o;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned v = rq(s[4 * t], div, p.scale, p.lo) | (rq(s[4 * t + 1], div, p.scale, p.lo) << 8) |
                               (rq(s[4 * t + 2], div, p.scale, p.lo) << 16) | (rq(s[4 * t + 3], div, p.scale, p.lo) << 24);
            o[t] = v & avg_dword_mask(g, c.k, t);
        }
        *reinterpret_cast<v4u*>(y + (size_t)i * 16) = o;
    }
}
extern "C" int avg16c_launch(const int16_t* x, int8_t* y, int N, int H, int W, int C, int Cpad, int kh, int kw, int sh, int sw, int ph,
                             int pw, int cip, int shift, int relu, void* stream) {
    if (N <= 0 || (Cpad & 15) || C > Cpad || 2L * N * H * W * Cpad >= 0x7fffffffL || !x || !y) return -1;
    P16 p; AvgGeom& g = p.g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.Cpad = Cpad; g.CH = Cpad / 16; g.P = avg_out_size(H, kh, sh, ph); g.Q = avg_out_size(W, kw, sw, pw);
    if (g.P < 1 || g.Q < 1 || kh * kw > kAvgMaxTaps) return -1;
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw; g.cip = cip ? 1 : 0;
    g.nchunks = (unsigned)((long)N * g.P * g.Q * g.CH);
    p.scale = ldexpf(1.0f, shift); p.lo = relu ? 0.0f : -128.0f;
    avgpool_i16_c16_kernel<<<(unsigned)avg_blocks(g), kAvgBlock, 0, (hipStream_t)stream>>>(x, y, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
