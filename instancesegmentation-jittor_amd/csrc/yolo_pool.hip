// yolo_pool.hip -- darknet's [maxpool] and the SPP block of yolov3-spp as one launch ([UPSTREAM-RECALL] the public yolov3-tiny.cfg /
// yolov3-spp.cfg and darknet's maxpool_layer.c, unverified).  NHWC fp32, one 16-byte access per thread and channel quad.
//
// Geometry (both integer divisions): out = (H - 1) / stride + 1; the window of output o covers the inputs o * stride - (size - 1) / 2 + [0, size).  An even
// size therefore pads on the bottom / right only: tiny's size 2, stride 1 layer reads rows o and o + 1.
// Maximum: m = -inf; m = v > m ? v : m over the taps -- maxpool_kernel's (csrc/spatial.hip): the largest non-NaN tap, -inf where there is none.  As a VALUE
// that does not depend on the visiting order (only the sign of a zero maximum does, where a window holds zeros of both signs).
// zero_pad 0 (darknet): a tap outside the map is skipped.  zero_pad 1 (the PyTorch ports' ZeroPad2d + MaxPool2d): it contributes +0.0f.  Since the maximum
// above is an order-free fold over the multiset of taps, zero_pad 1 equals fold(zero_pad 0's result, +0.0f) exactly where the window leaves the map:
// both kernels compute that.
//
// spp_concat: out[n][y][x] = [mp13 | mp9 | mp5 | x] (darknet's route layers = -1, -3, -5, -6), stride 1.  A block owns one image and a slab of S channels
// (S = 16, or 8 where the plane H * W * 16 floats does not fit SPP_PLANE: maps over 22 x 22) and holds the slab's whole plane in LDS twice (a, t).  The
// launch is a chain of seven barriers on a few KB of data, so it is bound by latency, not bytes: 1024 threads (one or two items a thread per pass) and
// narrow slabs (more blocks) measured 3.4x faster at 13 x 13 x 512, bs = 1, than 256 threads on 32-channel slabs (DESIGN.md 21 has the table).  x is read from HBM once,
// written to the last quarter on the way in, and then
//     mp5 = col5(row5(x)),  mp9 = col5(row5(mp5)),  mp13 = col5(row5(mp9))           (row5 / col5: the clipped 5-tap maximum along x / y)
// 30 LDS taps per output set instead of 275.  Proof of the cascade under clipping: the clipped window of mp5 at p is [p - 2, p + 2] n [0, L); the union of
// those windows over p' in [p - 2, p + 2] n [0, L) is [p - 4, p + 4] n [0, L) -- the nearest in-range p' to each end carries it -- so mp5 o mp5 folds exactly
// the taps of the clipped mp9, each at least once, and an all-NaN inner window hands on -inf, the fold's identity.  The same step gives mp13 = mp5 o mp9,
// and a 2-D clipped window is the product of its 1-D windows.  The LDS planes always carry the zero_pad 0 values; under zero_pad 1 the +0.0f is folded
// in at the store of an output whose own K x K window leaves the map, which is the equality stated above, so no identity about padded cascades is used.
#include "../../include/isegmi.h"
#include "common.h"
#include "tail_launch.h"

namespace isegmi {

namespace {

constexpr int SPP_NT = 1024;
constexpr int SPP_PLANE = 8192;   // floats of one LDS plane: 32 x 32 x 8; 19 x 19 x 16 = 5776, 13 x 13 x 16 = 2704

__device__ __forceinline__ void fold4(float4& m, const float4 v) {
    m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y;
    m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
}

__global__ __launch_bounds__(256) void maxpool_darknet_kernel(const float* __restrict__ in, int N, int H, int W, int C, int size, int stride, int zero_pad,
                                                              int Ho, int Wo, float* __restrict__ out) {
    const int c4n = C >> 2, off = (size - 1) / 2;
    const int64_t total = (int64_t)N * Ho * Wo * c4n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        int64_t t = i / c4n;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const int h0 = ho * stride - off, w0 = wo * stride - off;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int r = 0; r < size; ++r) {
            const int hi = h0 + r;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int q = 0; q < size; ++q) {
                const int wi = w0 + q;
                if ((unsigned)wi >= (unsigned)W) continue;
                fold4(m, *(const float4*)(in + (((int64_t)n * H + hi) * W + wi) * C + c4 * 4));
            }
        }
        if (zero_pad && (h0 < 0 || w0 < 0 || h0 + size > H || w0 + size > W)) fold4(m, make_float4(0.f, 0.f, 0.f, 0.f));
        *(float4*)(out + (((int64_t)n * Ho + ho) * Wo + wo) * C + c4 * 4) = m;
    }
}

// grid = N * (C4 / S4); S4 = 1 << s4_log2: the slab in channel quads.  np * S4 <= SPP_PLANE / 4 (the launcher's choice of S4).
__global__ __launch_bounds__(SPP_NT) void spp_concat_kernel(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4, int s4_log2,
                                                            int zero_pad) {
    __shared__ float4 a[SPP_PLANE / 4];
    __shared__ float4 t[SPP_PLANE / 4];
    const int S4 = 1 << s4_log2, slabs = C4 >> s4_log2;
    const int n = (int)blockIdx.x / slabs, slab = (int)blockIdx.x - n * slabs;
    const int np = H * W, ne = np << s4_log2;
    const float4* src = in + (int64_t)n * np * C4 + slab * S4;
    float4* dst = out + (int64_t)n * np * 4 * C4 + slab * S4;
    for (int i = threadIdx.x; i < ne; i += SPP_NT) {
        const int pix = i >> s4_log2, q = i & (S4 - 1);
        const float4 v = src[(int64_t)pix * C4 + q];
        a[i] = v;
        dst[(int64_t)pix * 4 * C4 + 3 * C4 + q] = v;
    }
    __syncthreads();
    const int rs = W << s4_log2;   // one map row in LDS, in quads
#pragma unroll 1
    for (int stage = 0; stage < 3; ++stage) {   // K = 5, 9, 13 -> quarter 2, 1, 0
        for (int i = threadIdx.x; i < ne; i += SPP_NT) {
            const int pix = i >> s4_log2;
            const int x = pix % W;
            float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if ((unsigned)(x + d) < (unsigned)W) fold4(m, a[i + d * S4]);
            t[i] = m;
        }
        __syncthreads();
        const int r = 2 * stage + 2;   // K / 2
        for (int i = threadIdx.x; i < ne; i += SPP_NT) {
            const int pix = i >> s4_log2, q = i & (S4 - 1);
            const int y = pix / W, x = pix - y * W;
            float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if ((unsigned)(y + d) < (unsigned)H) fold4(m, t[i + d * rs]);
            a[i] = m;   // the next stage's input: always the zero_pad 0 value
            if (zero_pad && (x < r || y < r || x + r >= W || y + r >= H)) fold4(m, make_float4(0.f, 0.f, 0.f, 0.f));
            dst[(int64_t)pix * 4 * C4 + (2 - stage) * C4 + q] = m;
        }
        __syncthreads();
    }
}

inline unsigned pool_grid(int64_t total) {
    int64_t b = cdiv64(total, 256);
    return (unsigned)(b > 2048 ? 2048 : b < 1 ? 1 : b);
}

}  // namespace

int maxpool_darknet_launch(const float* in, int N, int H, int W, int C, int size, int stride, int zero_pad, float* out, hipStream_t st) {
    ARG_CHECK(in && out, "maxpool_darknet: null pointer");
    ARG_CHECK(N >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "maxpool_darknet sizes");
    ARG_CHECK(C >= 4 && C % 4 == 0, "maxpool_darknet: C is a positive multiple of 4");
    ARG_CHECK(size >= 1 && size <= 13, "maxpool_darknet: size must be 1..13");
    ARG_CHECK(stride >= 1 && stride <= 2, "maxpool_darknet: stride must be 1 or 2");
    ARG_CHECK(zero_pad == 0 || zero_pad == 1, "maxpool_darknet: zero_pad is 0 or 1");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    hipLaunchKernelGGL(maxpool_darknet_kernel, dim3(pool_grid((int64_t)N * Ho * Wo * (C / 4))), dim3(256), 0, st, in, N, H, W, C, size, stride, zero_pad, Ho,
                       Wo, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int spp_concat_launch(const float* in, int N, int H, int W, int C, int zero_pad, float* out, hipStream_t st) {
    ARG_CHECK(in && out, "spp_concat: null pointer");
    ARG_CHECK(N >= 1 && H >= 1 && W >= 1 && H <= 32 && W <= 32, "spp_concat: the map is 1..32 x 1..32 (the stride-32 map of a canvas up to 1024)");
    ARG_CHECK(C >= 32 && C % 32 == 0, "spp_concat: C is a positive multiple of 32");
    ARG_CHECK(zero_pad == 0 || zero_pad == 1, "spp_concat: zero_pad is 0 or 1");
    const int s4_log2 = ((H * W * 4) << 2) <= SPP_PLANE ? 2 : 1;   // 16 channels, or 8: 32 x 32 x 8 floats fit
    const int64_t blocks = (int64_t)N * ((C / 4) >> s4_log2);
    ARG_CHECK(blocks <= 0x7fffffff, "spp_concat: too many slabs for one launch");
    hipLaunchKernelGGL(spp_concat_kernel, dim3((unsigned)blocks), dim3(SPP_NT), 0, st, (const float4*)in, (float4*)out, H, W, C / 4, s4_log2, zero_pad);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_maxpool_darknet(const float* d_in, int N, int H, int W, int C, int size, int stride, int zero_pad, float* d_out, void* stream) {
    return maxpool_darknet_launch(d_in, N, H, W, C, size, stride, zero_pad, d_out, (hipStream_t)stream);
}
extern "C" int isegmi_op_spp_concat(const float* d_in, int N, int H, int W, int C, int zero_pad, float* d_out, void* stream) {
    return spp_concat_launch(d_in, N, H, W, C, zero_pad, d_out, (hipStream_t)stream);
}
