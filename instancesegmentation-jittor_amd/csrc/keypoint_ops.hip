// keypoint_ops.hip -- the tail of the Keypoint R-CNN head ([UPSTREAM-RECALL] roi_heads/keypoint_head): the predictor's pixel shuffle +
// bilinear x2, and Keypointer's heatmaps_to_keypoints as ONE fused "bicubic resize + arg-max" launch that never writes the resized map.
// Every product and sum below is its own fp32 operation (the library is built with -ffp-contract=off); tests/keypoint_ref.py restates them in numpy.
#include <limits.h>

#include "../../include/isegmi.h"
#include "common.h"
#include "detmath.h"
#include "tail_launch.h"

namespace isegmi {

// ConvTranspose2d(4, 2, 1) ran as a 3x3 convolution with 4 * K outputs (parity-major: channel (2 py + px) * K + k); the low-resolution map is its pixel
// shuffle, lr[2y + py][2x + px][k], read in place.  out = interpolate(lr, scale_factor 2, bilinear, align_corners False) with resize_bilinear_kernel's
// coefficients and rounding sequence (dm_bil_coef, dm_bil1): bit-identical to "shuffle, then isegmi_op_resize_bilinear".
__global__ void keypoint_heatmap_kernel(const float* __restrict__ in, int64_t R, int Hi, int Wi, int K, float* __restrict__ out) {
    const int Hl = 2 * Hi, Wl = 2 * Wi, Ho = 4 * Hi, Wo = 4 * Wi;
    const int64_t total = R * Ho * Wo * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        int64_t t = i / K;
        const int x = (int)(t % Wo); t /= Wo;
        const int y = (int)(t % Ho);
        const int64_t r = t / Ho;
        int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
        dm_bil_coef(y, Hl, Ho, y0, y1, ly0, ly1);
        dm_bil_coef(x, Wl, Wo, x0, x1, lx0, lx1);
        const float* b = in + r * Hi * Wi * 4 * K + k;
        auto lr = [&](int Y, int X) { return b[((int64_t)(Y >> 1) * Wi + (X >> 1)) * 4 * K + ((Y & 1) * 2 + (X & 1)) * K]; };
        out[i] = dm_bil1(lx0, lx1, ly0, ly1, lr(y0, x0), lr(y0, x1), lr(y1, x0), lr(y1, x1));
    }
}

constexpr int KP_MAX_S = 64;         // side of the heat map staged in LDS (56 in the model)
constexpr int KP_MAX_SIDE = 16384;   // resized side beyond which a box is outside the contract (the engine's boxes are clipped to the canvas)
constexpr int KP_THREADS = 256;

// cv2.INTER_CUBIC / torch bicubic, align_corners False: A = -0.75, half-pixel centres, taps clamped to the map
__device__ __forceinline__ void kp_cubic(int d, float scale, int n_in, int& s, float w[4]) {
    const float f = ((float)d + 0.5f) * scale - 0.5f;
    const float sf = floorf(f);
    const float t = f - sf, u = 1.0f - t, x = t + 1.0f;
    constexpr float A = -0.75f, A5 = 5.0f * A, A8 = 8.0f * A, A4 = 4.0f * A, A2 = A + 2.0f, A3 = A + 3.0f;   // all exact in fp32
    s = (int)sf;
    w[0] = ((A * x - A5) * x + A8) * x - A4;
    w[1] = ((A2 * t - A3) * t) * t + 1.0f;
    w[2] = ((A2 * u - A3) * u) * u + 1.0f;
    w[3] = ((1.0f - w[0]) - w[1]) - w[2];
}
__device__ __forceinline__ int kp_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// np.argmax's order: a NaN is maximal; otherwise the larger value wins; equal values (as floats: -0 == +0) and two NaNs: the lower row-major position.
// (bv, bp) starts as (-inf, INT_MAX), which loses to every position, an all -inf map's included.
__device__ __forceinline__ void kp_better(float v, int p, float& bv, int& bp) {
    const bool nan = v != v;
    if (v > bv || ((v == bv || nan) && p < bp) || (nan && bv == bv)) { bv = v; bp = p; }
}

// One workgroup per (detection slot, keypoint).  The keypoint's S x S map sits in LDS; a thread owns output columns (their four horizontal taps and weights
// are fixed) and walks down its rows with the four horizontally interpolated source rows of the current vertical window in registers: moving one source row
// down costs one new row value, so an enlarged map costs about one vertical pass per output position.  Narrow boxes split their rows over the idle threads.
__global__ __launch_bounds__(KP_THREADS) void keypoint_decode_kernel(const float* __restrict__ heat, const float* __restrict__ boxes, const int* __restrict__ count,
                                                                      int cap, int S, int K, float* __restrict__ kpt, float* __restrict__ kscore) {
    __shared__ float m[KP_MAX_S * KP_MAX_S];
    __shared__ float red_v[KP_THREADS / 64];
    __shared__ int red_p[KP_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int64_t r = blockIdx.y;
    float* okp = kpt + (r * K + k) * 3;
    if ((int)(r % cap) >= count[r / cap]) {   // an empty slot: zeros, and its heat map is not read
        if (tid < 3) okp[tid] = 0.0f;
        if (tid == 3) kscore[r * K + k] = 0.0f;
        return;
    }
    for (int i = tid; i < S * S; i += KP_THREADS) m[i] = heat[(r * S * S + i) * K + k];
    const float x1 = boxes[r * 4], y1 = boxes[r * 4 + 1];
    const float w = fmaxf(boxes[r * 4 + 2] - x1, 1.0f), h = fmaxf(boxes[r * 4 + 3] - y1, 1.0f);
    const float wcf = fminf(ceilf(w), (float)KP_MAX_SIDE), hcf = fminf(ceilf(h), (float)KP_MAX_SIDE);
    const int wc = (int)wcf, hc = (int)hcf;
    const float sx = dm_div((float)S, wcf), sy = dm_div((float)S, hcf);
    __syncthreads();

    const int ncol = wc < KP_THREADS ? wc : KP_THREADS, nseg = KP_THREADS / ncol;
    const int rows_per = (hc + nseg - 1) / nseg;
    const int lane = tid % ncol, seg = tid / ncol;
    const int ya = seg * rows_per, yb = seg < nseg ? (ya + rows_per < hc ? ya + rows_per : hc) : 0;
    float bv = -INFINITY;
    int bp = INT_MAX;
    for (int x = lane; x < wc && ya < yb; x += ncol) {
        int s;
        float wx[4], wy[4];
        kp_cubic(x, sx, S, s, wx);
        const int c0 = kp_clamp(s - 1, S), c1 = kp_clamp(s, S), c2 = kp_clamp(s + 1, S), c3 = kp_clamp(s + 2, S);
        auto hrow = [&](int yy) {
            const float* q = m + kp_clamp(yy, S) * S;
            return ((wx[0] * q[c0] + wx[1] * q[c1]) + wx[2] * q[c2]) + wx[3] * q[c3];
        };
        int cur = INT_MIN;
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
        for (int y = ya; y < yb; ++y) {
            kp_cubic(y, sy, S, s, wy);
            if (s != cur) {
                if (s == cur + 1) { r0 = r1; r1 = r2; r2 = r3; r3 = hrow(s + 2); }
                else { r0 = hrow(s - 1); r1 = hrow(s); r2 = hrow(s + 1); r3 = hrow(s + 2); }
                cur = s;
            }
            const float v = ((wy[0] * r0 + wy[1] * r1) + wy[2] * r2) + wy[3] * r3;
            kp_better(v, y * wc + x, bv, bp);
        }
    }
    for (int o = 32; o > 0; o >>= 1) kp_better(__shfl_xor(bv, o, 64), __shfl_xor(bp, o, 64), bv, bp);
    if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_p[tid >> 6] = bp; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < KP_THREADS / 64; ++i) kp_better(red_v[i], red_p[i], bv, bp);
        const int xi = bp % wc, yi = bp / wc;
        const float cw = dm_div(w, wcf), ch = dm_div(h, hcf);
        okp[0] = ((float)xi + 0.5f) * cw + x1;
        okp[1] = ((float)yi + 0.5f) * ch + y1;
        okp[2] = 1.0f;
        kscore[r * K + k] = bv;
    }
}

int keypoint_heatmap_launch(const float* in, int64_t R, int Hi, int Wi, int K, float* out, hipStream_t st) {
    ARG_CHECK(in && out && R >= 0 && Hi > 0 && Wi > 0 && K > 0, "keypoint_heatmap args");
    if (R == 0) return ISEGMI_OK;
    const int64_t total = R * 16 * Hi * Wi * K, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(keypoint_heatmap_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, in, R, Hi, Wi, K, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int keypoint_decode_launch(const float* heat, const float* boxes, const int* count, int N, int cap, int S, int K, float* kpt, float* kscore, hipStream_t st) {
    ARG_CHECK(heat && boxes && count && kpt && kscore, "keypoint_decode: null");
    ARG_CHECK(N > 0 && cap > 0 && (int64_t)N * cap <= 65535, "keypoint_decode: N * cap must be 1..65535");
    ARG_CHECK(S >= 1 && S <= KP_MAX_S, "keypoint_decode: heat-map side 1..64");
    ARG_CHECK(K >= 1 && K <= 32, "keypoint_decode: 1..32 keypoints");
    hipLaunchKernelGGL(keypoint_decode_kernel, dim3(K, N * cap), dim3(KP_THREADS), 0, st, heat, boxes, count, cap, S, K, kpt, kscore);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

extern "C" int isegmi_op_keypoint_heatmap(const float* d_in, int64_t R, int Hi, int Wi, int K, float* d_out, void* stream) {
    return isegmi::keypoint_heatmap_launch(d_in, R, Hi, Wi, K, d_out, (hipStream_t)stream);
}

extern "C" int isegmi_op_keypoint_decode(const float* d_heat, const float* d_boxes, const int32_t* d_count, int N, int cap, int S, int K, float* d_kpt,
                                         float* d_kscore, void* stream) {
    return isegmi::keypoint_decode_launch(d_heat, d_boxes, d_count, N, cap, S, K, d_kpt, d_kscore, (hipStream_t)stream);
}
