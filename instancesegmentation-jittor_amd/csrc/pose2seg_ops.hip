// pose2seg_ops.hip -- the pose-specific stages of Pose2Seg: the input letterbox, the per-instance pose template
// fit, the Affine-Align sampler, the skeleton feature renderer and the fused softmax + reverse affine warp that pastes every 64 x 64
// prediction back at its image's own size.  fp32 storage; the fit runs in fp64.  Every result is a pure function of its inputs: the
// restatement in tests/pose2seg_ref.py follows the same operation order, and the GPU tests compare the two bit for bit.
#include "../../include/isegmi.h"
#include "common.h"
#include "detmath.h"

namespace isegmi {

constexpr int kP2sAlign = 64;    // size_align = size_output
constexpr int kP2sJoints = 17;
constexpr int kP2sLimbs = 19;
constexpr int kP2sMaxTemplates = 64;

// the COCO person skeleton, 0-based (upstream lists it 1-based)
__constant__ int8_t c_p2s_limbs[kP2sLimbs][2] = {{15, 13}, {13, 11}, {16, 14}, {14, 12}, {11, 12}, {5, 11}, {6, 12}, {5, 6}, {5, 7}, {6, 8},
                                                  {7, 9},   {8, 10},  {1, 2},   {0, 1},   {0, 2},   {1, 3},  {2, 4},  {3, 5}, {4, 6}};

// The one bilinear helper of the three warps: taps (x0, y0) .. (x0 + 1, y0 + 1), zero outside [0, W) x [0, H).  A sample outside
// (-1, W) x (-1, H) (or NaN) touches no tap at all and gives +0, what its four zero taps would give.
struct Bil {
    int x0, y0;
    float wx0, wx1, wy0, wy1;
    bool any;
};
__device__ __forceinline__ Bil bil_setup(float sx, float sy, int W, int H) {
    Bil b;
    b.any = sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H;
    const float fx = b.any ? floorf(sx) : 0.0f, fy = b.any ? floorf(sy) : 0.0f;
    b.x0 = (int)fx; b.y0 = (int)fy;
    b.wx1 = sx - fx; b.wx0 = 1.0f - b.wx1;
    b.wy1 = sy - fy; b.wy0 = 1.0f - b.wy1;
    return b;
}
__device__ __forceinline__ float bil_mix(float v00, float v01, float v10, float v11, const Bil& b) {
    return ((v00 * b.wx0 + v01 * b.wx1) * b.wy0) + ((v10 * b.wx0 + v11 * b.wx1) * b.wy1);
}

// ---------------------------------------------------------------- 1. letterbox (m1) + normalise -> NHWC4 stem input
struct P2sNorm {
    float mean[3], std[3];
};

__global__ void __launch_bounds__(256) p2s_letterbox_kernel(const uint8_t* __restrict__ src, const isegmi_p2s_image* __restrict__ table, int N, int S,
                                                            P2sNorm nm, int swap_rb, int round_u8, float4* __restrict__ out) {
    const int64_t total = (int64_t)N * S * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / ((int64_t)S * S));
        const int p = (int)(i - (int64_t)n * S * S);
        const float x = (float)(p % S), y = (float)(p / S);
        const isegmi_p2s_image im = table[n];
        const float sx = (im.minv[0] * x + im.minv[1] * y) + im.minv[2];
        const float sy = (im.minv[3] * x + im.minv[4] * y) + im.minv[5];
        const Bil b = bil_setup(sx, sy, im.w, im.h);
        const uint8_t* img = src + im.offset;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (b.any) {
            const bool xa = b.x0 >= 0, xb = b.x0 + 1 < im.w, ya = b.y0 >= 0, yb = b.y0 + 1 < im.h;
            for (int c = 0; c < 3; ++c) {
                const float v00 = ya && xa ? (float)img[((int64_t)b.y0 * im.w + b.x0) * 3 + c] : 0.0f;
                const float v01 = ya && xb ? (float)img[((int64_t)b.y0 * im.w + b.x0 + 1) * 3 + c] : 0.0f;
                const float v10 = yb && xa ? (float)img[((int64_t)(b.y0 + 1) * im.w + b.x0) * 3 + c] : 0.0f;
                const float v11 = yb && xb ? (float)img[((int64_t)(b.y0 + 1) * im.w + b.x0 + 1) * 3 + c] : 0.0f;
                v[c] = bil_mix(v00, v01, v10, v11, b);
            }
        }
        float o[3];
        for (int c = 0; c < 3; ++c) {
            float t = v[swap_rb ? 2 - c : c];
            if (round_u8) t = fminf(fmaxf(floorf(t + 0.5f), 0.0f), 255.0f);
            o[c] = dm_div(dm_div(t, 255.0f) - nm.mean[c], nm.std[c]);
        }
        out[i] = make_float4(o[0], o[1], o[2], 0.0f);
    }
}

// ---------------------------------------------------------------- 2. pose template fit (m3) and the matrices derived from it, fp64
// 3 x 3 row-major helpers; every sum is written left to right, as the restatement writes it
__device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}
// adjugate (transposed cofactors); returns the determinant
__device__ __forceinline__ double mat3_adj(const double* m, double* adj) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double c10 = m[2] * m[7] - m[1] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[1] * m[6] - m[0] * m[7];
    const double c20 = m[1] * m[5] - m[2] * m[4], c21 = m[2] * m[3] - m[0] * m[5], c22 = m[0] * m[4] - m[1] * m[3];
    adj[0] = c00; adj[1] = c10; adj[2] = c20;
    adj[3] = c01; adj[4] = c11; adj[5] = c21;
    adj[6] = c02; adj[7] = c12; adj[8] = c22;
    return (m[0] * c00 + m[1] * c01) + m[2] * c02;
}

// one block per instance, one thread per template; thread 0 takes the argmin and writes the instance's matrices
__global__ void __launch_bounds__(64) p2s_fit_kernel(const float* __restrict__ kpts, const int32_t* __restrict__ roi_img, const double* __restrict__ m1s,
                                                     const float* __restrict__ tmpl, int T, int align_corners, float* __restrict__ m3_out,
                                                     float* __restrict__ g_out, float* __restrict__ mmask_out, float* __restrict__ kal_out,
                                                     double* __restrict__ fit_out) {
    __shared__ double s_kx[kP2sJoints], s_ky[kP2sJoints];
    __shared__ float s_v[kP2sJoints];
    __shared__ double s_A[kP2sMaxTemplates][6];
    __shared__ double s_err[kP2sMaxTemplates];
    __shared__ int s_ok[kP2sMaxTemplates];
    __shared__ double s_m21[9];
    const int r = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        const double* m1v = m1s + (int64_t)roi_img[r] * 6;
        const double m1[9] = {m1v[0], m1v[1], m1v[2], m1v[3], m1v[4], m1v[5], 0.0, 0.0, 1.0};
        const double m2[9] = {0.25, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0};
        mat3_mul(m2, m1, s_m21);
    }
    __syncthreads();
    if (t < kP2sJoints) {
        const float* k = kpts + ((int64_t)r * kP2sJoints + t) * 3;
        const double x = (double)k[0], y = (double)k[1];
        s_kx[t] = (s_m21[0] * x + s_m21[1] * y) + s_m21[2];
        s_ky[t] = (s_m21[3] * x + s_m21[4] * y) + s_m21[5];
        s_v[t] = isfinite(k[0]) && isfinite(k[1]) ? k[2] : 0.0f;   // a non-finite coordinate counts as not visible
    }
    __syncthreads();
    if (t < T) {
        double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, B[6] = {0, 0, 0, 0, 0, 0};
        double wsum = 0.0;
        int n = 0;
        const float* tp = tmpl + (int64_t)t * kP2sJoints * 3;
        for (int j = 0; j < kP2sJoints; ++j) {
            const double w = (double)tp[j * 3 + 2];
            if (!(s_v[j] > 0.0f) || !(w > 0.0)) continue;
            const double p[3] = {s_kx[j], s_ky[j], 1.0};
            const double qx = (double)tp[j * 3], qy = (double)tp[j * 3 + 1];
            for (int a = 0; a < 3; ++a) {
                const double wp = w * p[a];
                for (int c = 0; c < 3; ++c) S[a * 3 + c] = S[a * 3 + c] + wp * p[c];
                B[a * 2] = B[a * 2] + wp * qx;
                B[a * 2 + 1] = B[a * 2 + 1] + wp * qy;
            }
            wsum = wsum + w;
            ++n;
        }
        double adj[9];
        const double det = mat3_adj(S, adj);
        const double tr = (S[0] + S[4]) + S[8];
        int ok = n >= 3 && fabs(det) > 1e-9 * tr * tr * tr;
        double A[6] = {0, 0, 0, 0, 0, 0}, err = 0.0;
        if (ok) {
            // X = adj(S) B / det is [3][2]; row k of the affine is column k of X
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 2; ++k) A[k * 3 + i] = ((adj[i * 3] * B[k] + adj[i * 3 + 1] * B[2 + k]) + adj[i * 3 + 2] * B[4 + k]) / det;
            for (int j = 0; j < kP2sJoints; ++j) {
                const double w = (double)tp[j * 3 + 2];
                if (!(s_v[j] > 0.0f) || !(w > 0.0)) continue;
                const double rx = ((A[0] * s_kx[j] + A[1] * s_ky[j]) + A[2]) - (double)tp[j * 3];
                const double ry = ((A[3] * s_kx[j] + A[4] * s_ky[j]) + A[5]) - (double)tp[j * 3 + 1];
                err = err + w * (rx * rx + ry * ry);
            }
            err = err / wsum;
            ok = err == err;
        }
        for (int i = 0; i < 6; ++i) s_A[t][i] = A[i];
        s_err[t] = err;
        s_ok[t] = ok;
    }
    __syncthreads();
    if (t != 0) return;
    int best = -1;
    for (int u = 0; u < T; ++u)
        if (s_ok[u] && (best < 0 || s_err[u] < s_err[best])) best = u;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1.0};
    double err = 0.0;
    if (best >= 0) {
        for (int i = 0; i < 6; ++i) H[i] = s_A[best][i];
        err = s_err[best];
    } else {
        // fallback (this engine's contract): the visible keypoints' box, squared to max(bw, bh) * 1.2 (>= 8 px), centred on the 64 x 64 frame;
        // no visible keypoint: the whole 128 x 128 map at scale 1/2
        int nv = 0;
        double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        for (int j = 0; j < kP2sJoints; ++j) {
            if (!(s_v[j] > 0.0f)) continue;
            if (nv == 0) { x0 = x1 = s_kx[j]; y0 = y1 = s_ky[j]; }
            else { x0 = fmin(x0, s_kx[j]); x1 = fmax(x1, s_kx[j]); y0 = fmin(y0, s_ky[j]); y1 = fmax(y1, s_ky[j]); }
            ++nv;
        }
        if (nv == 0) {
            H[0] = 0.5; H[4] = 0.5;
        } else {
            double side = fmax(x1 - x0, y1 - y0) * 1.2;
            if (side < 8.0) side = 8.0;
            const double k = 64.0 / side;
            const double cx = (x0 + x1) * 0.5, cy = (y0 + y1) * 0.5;
            H[0] = k; H[2] = 32.0 - k * cx;
            H[4] = k; H[5] = 32.0 - k * cy;
        }
    }
    // Affine-Align: theta = inv(A H A^-1) on the normalised 128 x 128 grid, folded with the grid's normalise / unnormalise into a pixel-space G
    const double An[9] = {2.0 / 128.0, 0.0, -1.0, 0.0, 2.0 / 128.0, -1.0, 0.0, 0.0, 1.0};
    const double Ai[9] = {64.0, 0.0, 64.0, 0.0, 64.0, 64.0, 0.0, 0.0, 1.0};
    double AH[9], M[9], adj[9], theta[9];
    mat3_mul(An, H, AH);
    mat3_mul(AH, Ai, M);
    const double dM = mat3_adj(M, adj);
    for (int i = 0; i < 9; ++i) theta[i] = adj[i] / dM;
    const double nsc = align_corners ? 2.0 / 127.0 : 2.0 / 128.0, nof = align_corners ? -1.0 : 1.0 / 128.0 - 1.0;
    const double usc = align_corners ? 63.5 : 64.0;
    const double Nrm[9] = {nsc, 0.0, nof, 0.0, nsc, nof, 0.0, 0.0, 1.0};
    const double Un[9] = {usc, 0.0, 63.5, 0.0, usc, 63.5, 0.0, 0.0, 1.0};
    double TN[9], G[9], Mm[9];
    mat3_mul(theta, Nrm, TN);
    mat3_mul(Un, TN, G);
    mat3_mul(H, s_m21, Mm);   // Mmask = m4 m3 m2 m1, m4 = I
    for (int i = 0; i < 6; ++i) {
        m3_out[r * 6 + i] = (float)H[i];
        g_out[r * 6 + i] = (float)G[i];
        mmask_out[r * 6 + i] = (float)Mm[i];
        fit_out[r * 8 + i] = H[i];
    }
    fit_out[r * 8 + 6] = err;
    fit_out[r * 8 + 7] = (double)best;
    for (int j = 0; j < kP2sJoints; ++j) {
        float* o = kal_out + ((int64_t)r * kP2sJoints + j) * 3;
        o[0] = (float)((H[0] * s_kx[j] + H[1] * s_ky[j]) + H[2]);
        o[1] = (float)((H[3] * s_kx[j] + H[4] * s_ky[j]) + H[5]);
        o[2] = s_v[j];
    }
}

// ---------------------------------------------------------------- 3. Affine-Align: NHWC P2 -> [R][64][64][out_c] channels [0, C)
// one float4 of channels per lane: a wave reads a 256-channel row (1 KiB) of every tap
__global__ void __launch_bounds__(256) p2s_align_kernel(const float* __restrict__ feat, int Hf, int Wf, int C, const int32_t* __restrict__ roi_img,
                                                        const float* __restrict__ G, int R, float* __restrict__ out, int out_c) {
    const int c4n = C / 4;
    const int64_t total = (int64_t)R * kP2sAlign * kP2sAlign * c4n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int64_t pix = i / c4n;
        const int r = (int)(pix / (kP2sAlign * kP2sAlign));
        const int p = (int)(pix - (int64_t)r * kP2sAlign * kP2sAlign);
        const float x = (float)(p % kP2sAlign), y = (float)(p / kP2sAlign);
        const float* g = G + r * 6;
        const float sx = (g[0] * x + g[1] * y) + g[2];
        const float sy = (g[3] * x + g[4] * y) + g[5];
        const Bil b = bil_setup(sx, sy, Wf, Hf);
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b.any) {
            const float4* f = (const float4*)(feat + (int64_t)roi_img[r] * Hf * Wf * C);
            const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const bool xa = b.x0 >= 0, xb = b.x0 + 1 < Wf, ya = b.y0 >= 0, yb = b.y0 + 1 < Hf;
            const float4 v00 = ya && xa ? f[((int64_t)b.y0 * Wf + b.x0) * c4n + c4] : z;
            const float4 v01 = ya && xb ? f[((int64_t)b.y0 * Wf + b.x0 + 1) * c4n + c4] : z;
            const float4 v10 = yb && xa ? f[((int64_t)(b.y0 + 1) * Wf + b.x0) * c4n + c4] : z;
            const float4 v11 = yb && xb ? f[((int64_t)(b.y0 + 1) * Wf + b.x0 + 1) * c4n + c4] : z;
            o.x = bil_mix(v00.x, v01.x, v10.x, v11.x, b);
            o.y = bil_mix(v00.y, v01.y, v10.y, v11.y, b);
            o.z = bil_mix(v00.z, v01.z, v10.z, v11.z, b);
            o.w = bil_mix(v00.w, v01.w, v10.w, v11.w, b);
        }
        *(float4*)(out + pix * out_c + c4 * 4) = o;
    }
}

// ---------------------------------------------------------------- 4. skeleton features: channels [c0, c0 + 55), zeros in [c0 + 55, c0 + 64)
// correctly rounded sqrt of a positive finite float: the hardware result (measured up to 1 ulp low on gfx950) is moved to the neighbour
// whose rounding interval holds s.  The midpoints' squares are exact in fp64 (25-bit operands), so every comparison is exact.
__device__ __forceinline__ float p2s_sqrt_rn(float s) {
    const float r = __fsqrt_rn(s);
    const float up = __uint_as_float(__float_as_uint(r) + 1u), dn = __uint_as_float(__float_as_uint(r) - 1u);
    const double ds = (double)s;
    const double mu = ((double)r + (double)up) * 0.5, md = ((double)dn + (double)r) * 0.5;
    if (ds > mu * mu) return up;
    if (ds < md * md) return dn;
    return r;
}

__global__ void __launch_bounds__(256) p2s_skeleton_kernel(const float* __restrict__ kal, int R, float* __restrict__ out, int out_c, int c0) {
    const int64_t total = (int64_t)R * kP2sAlign * kP2sAlign;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (kP2sAlign * kP2sAlign));
        const int p = (int)(i - (int64_t)r * kP2sAlign * kP2sAlign);
        const float x = (float)(p % kP2sAlign), y = (float)(p / kP2sAlign);
        const float* k = kal + (int64_t)r * kP2sJoints * 3;
        float v[64];
        for (int c = 0; c < 64; ++c) v[c] = 0.0f;
        for (int j = 0; j < kP2sJoints; ++j) {
            if (!(k[j * 3 + 2] > 0.0f)) continue;
            const float dx = x - k[j * 3], dy = y - k[j * 3 + 1];
            const float d2 = dx * dx + dy * dy;
            const float e = dm_div(dm_div(d2 * 0.5f, 3.0f), 3.0f);
            v[j] = e <= 4.6052f ? dm_exp(-e) : 0.0f;
        }
        for (int l = 0; l < kP2sLimbs; ++l) {
            const int a = c_p2s_limbs[l][0], bb = c_p2s_limbs[l][1];
            if (!(k[a * 3 + 2] > 0.0f) || !(k[bb * 3 + 2] > 0.0f)) continue;
            const float ax = k[a * 3], ay = k[a * 3 + 1], bx = k[bb * 3], by = k[bb * 3 + 1];
            const float lx = bx - ax, ly = by - ay;
            const float norm = p2s_sqrt_rn(lx * lx + ly * ly);
            if (!(norm > 0.0f)) continue;
            const float ux = dm_div(lx, norm), uy = dm_div(ly, norm);
            const float x_lo = fmaxf(rintf(fminf(ax, bx) - 1.0f), 0.0f), x_hi = fminf(rintf(fmaxf(ax, bx) + 1.0f), (float)kP2sAlign);
            const float y_lo = fmaxf(rintf(fminf(ay, by) - 1.0f), 0.0f), y_hi = fminf(rintf(fmaxf(ay, by) + 1.0f), (float)kP2sAlign);
            if (!(x >= x_lo && x < x_hi && y >= y_lo && y < y_hi)) continue;
            const float perp = (x - ax) * uy - (y - ay) * ux;
            if (fabsf(perp) < 1.0f) {
                v[kP2sJoints + 2 * l] = ux;
                v[kP2sJoints + 2 * l + 1] = uy;
            }
        }
        float4* o = (float4*)(out + i * out_c + c0);
        for (int q = 0; q < 16; ++q) o[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// ---------------------------------------------------------------- 5. softmax + reverse affine warp -> det.masks, tight boxes, scores, labels, counts
__global__ void p2s_masks_init_kernel(const int32_t* __restrict__ counts, int N, int K, int32_t* __restrict__ ws_box, float* __restrict__ scores,
                                      int32_t* __restrict__ labels, int32_t* __restrict__ count_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    const int n = i / K, k = i - n * K;
    const bool valid = k < counts[n];
    ws_box[i * 4] = 0x7fffffff; ws_box[i * 4 + 1] = 0x7fffffff;
    ws_box[i * 4 + 2] = -1; ws_box[i * 4 + 3] = -1;
    scores[i] = valid ? 1.0f : 0.0f;
    labels[i] = valid ? 1 : 0;
    if (k == 0) count_out[n] = counts[n];
}

constexpr int kP2sTile = 64;   // 64 x 64 image pixels per block of 256 threads: 16 rows of one column per thread
__global__ void __launch_bounds__(256) p2s_masks_kernel(const float* __restrict__ logits, const float* __restrict__ mmask, const int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ roi_off, const int32_t* __restrict__ image_hw, int K, int Hmax, int Wmax,
                                                        int32_t* __restrict__ ws_box, uint8_t* __restrict__ masks) {
    __shared__ float s_p[kP2sAlign * kP2sAlign];   // channel 1 of the softmax, 16 KiB
    __shared__ int s_box[4];
    const int slot = blockIdx.z, n = slot / K, k = slot - n * K;
    const int tx0 = blockIdx.x * kP2sTile, ty0 = blockIdx.y * kP2sTile;
    const int h = image_hw[n * 2], w = image_hw[n * 2 + 1];
    const bool live = k < counts[n] && tx0 < w && ty0 < h;   // uniform over the block
    uint8_t* plane = masks + (int64_t)slot * Hmax * Wmax;
    const int lx = threadIdx.x % kP2sTile, ly0 = threadIdx.x / kP2sTile;
    if (!live) {
        for (int q = 0; q < kP2sTile / 4; ++q) {
            const int x = tx0 + lx, y = ty0 + ly0 + 4 * q;
            if (x < Wmax && y < Hmax) plane[(int64_t)y * Wmax + x] = 0;
        }
        return;
    }
    const int r = roi_off[n] + k;
    const float2* lg = (const float2*)(logits + (int64_t)r * kP2sAlign * kP2sAlign * 2);
    for (int q = threadIdx.x; q < kP2sAlign * kP2sAlign; q += blockDim.x) {
        const float2 a = lg[q];   // ora_softmax order: max, exp, sum, divide
        const float m = a.y > a.x ? a.y : a.x;
        const float e0 = dm_exp(a.x - m);
        const float e1 = dm_exp(a.y - m);
        const float s = (0.0f + e0) + e1;
        s_p[q] = dm_div(e1, s);
    }
    if (threadIdx.x < 4) s_box[threadIdx.x] = threadIdx.x < 2 ? 0x7fffffff : -1;
    __syncthreads();
    const float* M = mmask + r * 6;
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -1, by1 = -1;
    for (int q = 0; q < kP2sTile / 4; ++q) {
        const int x = tx0 + lx, y = ty0 + ly0 + 4 * q;
        if (x >= Wmax || y >= Hmax) continue;
        uint8_t m = 0;
        if (x < w && y < h) {
            const float fx = (float)x, fy = (float)y;
            const float sx = (M[0] * fx + M[1] * fy) + M[2];
            const float sy = (M[3] * fx + M[4] * fy) + M[5];
            const Bil b = bil_setup(sx, sy, kP2sAlign, kP2sAlign);
            if (b.any) {
                const bool xa = b.x0 >= 0, xb = b.x0 + 1 < kP2sAlign, ya = b.y0 >= 0, yb = b.y0 + 1 < kP2sAlign;
                const float v00 = ya && xa ? s_p[b.y0 * kP2sAlign + b.x0] : 0.0f;
                const float v01 = ya && xb ? s_p[b.y0 * kP2sAlign + b.x0 + 1] : 0.0f;
                const float v10 = yb && xa ? s_p[(b.y0 + 1) * kP2sAlign + b.x0] : 0.0f;
                const float v11 = yb && xb ? s_p[(b.y0 + 1) * kP2sAlign + b.x0 + 1] : 0.0f;
                m = bil_mix(v00, v01, v10, v11, b) > 0.5f ? 1 : 0;
            }
        }
        plane[(int64_t)y * Wmax + x] = m;
        if (m) { bx0 = min(bx0, x); by0 = min(by0, y); bx1 = max(bx1, x); by1 = max(by1, y); }
    }
    if (bx1 >= 0) {
        atomicMin(&s_box[0], bx0); atomicMin(&s_box[1], by0);
        atomicMax(&s_box[2], bx1); atomicMax(&s_box[3], by1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_box[2] >= 0) {
        atomicMin(&ws_box[slot * 4], s_box[0]); atomicMin(&ws_box[slot * 4 + 1], s_box[1]);
        atomicMax(&ws_box[slot * 4 + 2], s_box[2]); atomicMax(&ws_box[slot * 4 + 3], s_box[3]);
    }
}

// tight box of the set pixels, xyxy with exclusive right / bottom edges (pycocotools toBbox: x1 = max x + 1); an empty mask gets (0, 0, 0, 0)
__global__ void p2s_masks_box_kernel(const int32_t* __restrict__ ws_box, int NK, float* __restrict__ boxes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NK) return;
    const bool any = ws_box[i * 4 + 2] >= 0;
    boxes[i * 4] = any ? (float)ws_box[i * 4] : 0.0f;
    boxes[i * 4 + 1] = any ? (float)ws_box[i * 4 + 1] : 0.0f;
    boxes[i * 4 + 2] = any ? (float)(ws_box[i * 4 + 2] + 1) : 0.0f;
    boxes[i * 4 + 3] = any ? (float)(ws_box[i * 4 + 3] + 1) : 0.0f;
}

static inline unsigned p2s_grid(int64_t total) {
    int64_t b = cdiv64(total, 256);
    if (b > 8192) b = 8192;
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_pose2seg_letterbox(const uint8_t* d_u8, const isegmi_p2s_image* d_table, int N, int S, const float* mean3, const float* std3,
                                            int swap_rb, int round_u8, float* d_out, void* stream) {
    ARG_CHECK(d_u8 && d_table && d_out && mean3 && std3, "null pointer");
    ARG_CHECK(N >= 1 && S >= 1 && S <= 8192, "batch / plane size");
    P2sNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean3[c]; nm.std[c] = std3[c]; }
    hipLaunchKernelGGL(p2s_letterbox_kernel, dim3(p2s_grid((int64_t)N * S * S)), dim3(256), 0, (hipStream_t)stream, d_u8, d_table, N, S, nm,
                       swap_rb ? 1 : 0, round_u8 ? 1 : 0, (float4*)d_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_pose2seg_fit(const float* d_kpts, const int32_t* d_roi_img, int R, const double* d_m1, const float* d_templates, int T,
                                      int align_corners, float* d_m3, float* d_G, float* d_mmask, float* d_kalign, double* d_fit, void* stream) {
    ARG_CHECK(R >= 0, "instance count");
    ARG_CHECK(T >= 1 && T <= kP2sMaxTemplates, "template count (1..64)");
    if (R == 0) return ISEGMI_OK;
    ARG_CHECK(d_kpts && d_roi_img && d_m1 && d_templates && d_m3 && d_G && d_mmask && d_kalign && d_fit, "null device pointer");
    hipLaunchKernelGGL(p2s_fit_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, d_kpts, d_roi_img, d_m1, d_templates, T, align_corners ? 1 : 0, d_m3, d_G,
                       d_mmask, d_kalign, d_fit);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_pose2seg_align(const float* d_feat, int Hf, int Wf, int C, const int32_t* d_roi_img, const float* d_G, int R, float* d_out,
                                        int out_c, void* stream) {
    ARG_CHECK(R >= 0 && Hf >= 1 && Wf >= 1, "sizes");
    ARG_CHECK(C >= 4 && C % 4 == 0 && out_c % 4 == 0 && out_c >= C, "channels: C % 4 == 0, out_c % 4 == 0, out_c >= C");
    if (R == 0) return ISEGMI_OK;
    ARG_CHECK(d_feat && d_roi_img && d_G && d_out, "null device pointer");
    hipLaunchKernelGGL(p2s_align_kernel, dim3(p2s_grid((int64_t)R * kP2sAlign * kP2sAlign * (C / 4))), dim3(256), 0, (hipStream_t)stream, d_feat, Hf, Wf, C,
                       d_roi_img, d_G, R, d_out, out_c);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_pose2seg_skeleton(const float* d_kalign, int R, float* d_out, int out_c, int c0, void* stream) {
    ARG_CHECK(R >= 0, "instance count");
    ARG_CHECK(c0 >= 0 && c0 % 4 == 0 && out_c == c0 + 64, "layout: the 55 skeleton channels and 9 zero channels end the row (out_c == c0 + 64, c0 % 4 == 0)");
    if (R == 0) return ISEGMI_OK;
    ARG_CHECK(d_kalign && d_out, "null device pointer");
    hipLaunchKernelGGL(p2s_skeleton_kernel, dim3(p2s_grid((int64_t)R * kP2sAlign * kP2sAlign)), dim3(256), 0, (hipStream_t)stream, d_kalign, R, d_out, out_c,
                       c0);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_pose2seg_masks(const float* d_logits, const float* d_mmask, const int32_t* d_counts, const int32_t* d_roi_off,
                                        const int32_t* d_image_hw, int N, int K, int Hmax, int Wmax, int32_t* d_ws_box, uint8_t* d_masks, float* d_boxes,
                                        float* d_scores, int32_t* d_labels, int32_t* d_count_out, void* stream) {
    ARG_CHECK(N >= 1 && K >= 1 && Hmax >= 1 && Wmax >= 1, "sizes");
    ARG_CHECK((int64_t)N * K <= 65535, "N * K <= 65535");
    ARG_CHECK(d_logits && d_mmask && d_counts && d_roi_off && d_image_hw && d_ws_box && d_masks && d_boxes && d_scores && d_labels && d_count_out,
              "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(p2s_masks_init_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, s, d_counts, N, K, d_ws_box, d_scores, d_labels, d_count_out);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(p2s_masks_kernel, dim3(cdiv(Wmax, kP2sTile), cdiv(Hmax, kP2sTile), N * K), dim3(256), 0, s, d_logits, d_mmask, d_counts, d_roi_off,
                       d_image_hw, K, Hmax, Wmax, d_ws_box, d_masks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(p2s_masks_box_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, s, d_ws_box, N * K, d_boxes);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}
