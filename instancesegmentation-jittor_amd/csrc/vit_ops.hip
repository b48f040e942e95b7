// vit_ops.hip -- the operators of the ViT engine that are not convolutions: multi-head self-attention, LayerNorm, GELU, the patch
// gather in front of the patch embedding and the softmax over the class logits.  All fp32, all with a fixed operation order: tests/vit_ref.py restates
// every one of them on the host and the GPU tests compare bits.  Finite inputs only: NaN / inf are outside every contract below.
//
// ATTENTION (vit_attention_kernel).  d_qkv is [N][T][3 D] as the qkv convolution wrote it, D = heads * 64; channel which * D + h * 64 + d belongs to
// head h (which = 0 q, 1 k, 2 v).  d_out is [N][T][D], head h at channels h * 64 ..: nothing is transposed on either side.  Per (image, head):
//     s_ij = (fmaf chain from +0 over d = 0..63 of q_i[d] * k_j[d]) * 0.125             (0.125 = fp32(1 / sqrt(64)); the product is exact)
//     m_i  = max_j s_ij
//     e_ij = dm_exp(s_ij - m_i)
//     l_i  = (c_0 + c_1) + (c_2 + c_3),  c_r = the chain e_ir + e_i(r+4) + e_i(r+8) + ... from +0 (ascending j, j = r mod 4)
//     p_ij = dm_div(e_ij, l_i)
//     o_i[d] = fmaf chain from +0 over j = 0..T-1 of p_ij * v_j[d]
// Both products run on v_mfma_f32_16x16x4_f32, whose accumulation is bit for bit the k-ordered fmaf chain (one rounding per product).
//
// Geometry.  A workgroup of W wavefronts (W = 4; 2 once the score tiles of 4 would not fit the LDS) takes 16 W consecutive queries of one (image, head);
// wavefront w owns the 16 queries q0 + 16 w ...  Its q fragment (16 registers) comes straight from global memory.  Keys travel through one LDS staging
// area in chunks of 32 rows, first all of K (row pitch 66 floats: the 16 x 4 operand read of a half-wave touches 32 different banks), then all of V
// (pitch 80: two consecutive rows sit 16 banks apart).  Rows past T are staged as zeros and never read from memory.  The wavefront's score tile
// [16][Tc + 2] (Tc = T rounded up to 32; pitch = 2 mod 32, again for the operand read) lives in LDS between the two products: scores, then e, then p in
// place.  Softmax rows are spread over 4 lanes each (lane l: row l / 4, keys l % 4, l % 4 + 4, ...), which is what fixes the sum order above.  Columns
// T .. Tc - 1 are set to p = 0 and excluded from max and sum, so the PV chain sees fmaf(0, 0, acc) = acc there.  Query rows past T are computed on zeros
// and never stored.
//
// LAYERNORM (vit_layer_norm_kernel): the numerics of groupnorm.hip on one row.  One wavefront per row of D <= 2048 floats (D % 4 == 0), the row in
// registers.  K = x[0]; d = x - K; lane l chains s1 += d, s2 += d * d in fp32 from +0 over its elements in ascending order (float4 slots l, l + 64, ...;
// x, y, z, w inside a slot); the 64 lane sums fold in fp64 as the tree s[l] += s[l + off], off = 32, 16 .. 1 (an xor butterfly: every lane ends with lane
// 0's bits); md = S1 / D, var = max(S2 / D - md^2, 0), m = fp32(md), rstd = fp32(1 / sqrt(var + eps)), all in fp64; y = ((d - m) * rstd) * gamma + beta,
// every operation rounded on its own.  Rows are x_stride / out_stride floats apart (the final norm runs on the class-token rows only); out may be x.
//
// GELU (vit_gelu_kernel), in place allowed.  gelu_tanh 0: y = (0.5 x) * (1 + dm_erf(x * fp32(1 / sqrt 2)));  gelu_tanh 1: y = (0.5 x) * (1 +
// dm_tanh(fp32(sqrt(2 / pi)) * (x + 0.044715 * ((x * x) * x)))).  Every multiplication and addition is rounded on its own.
//
// PATCHIFY: [N][H][W][3] -> [N][H / P][W / P][P * P * 3], element (py * P + px) * 3 + c of patch (gy, gx) = pixel (gy P + py, gx P + px), channel c.
//
// CLASS SOFTMAX (vit_softmax_kernel): one wavefront per row of n logits; m = max; e_j = dm_exp(x_j - m); lane l chains e_l + e_(l+64) + ... from +0, the
// lane sums fold as the tree above in fp32; prob_j = dm_div(e_j, sum).
#include "detmath.h"
#include "engine.h"

namespace isegmi {

namespace {

constexpr int AT_HD = 64;        // head dimension
constexpr int AT_KC = 32;        // keys per staged chunk
constexpr int AT_KP = 66;        // K chunk row pitch (floats)
constexpr int AT_VP = 80;        // V chunk row pitch
constexpr int AT_STAGE = AT_KC * AT_VP;   // floats of the staging area (the larger of the two images)
constexpr int AT_LDS_MAX = 160 * 1024;
constexpr int LN_MAX_SLOTS = 8;  // float4 slots per lane: D <= 2048

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) vit_attention_kernel(const float* __restrict__ qkv, int T, int heads, int Tc, float* __restrict__ out) {
    extern __shared__ float lds[];
    const int SP = Tc + 2;
    const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lg = lane >> 4;
    const int h = blockIdx.y, n = blockIdx.z;
    const int D = heads * AT_HD;
    const int64_t row3 = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)n * T * row3 + h * AT_HD;   // q of (n, token 0, head h); k at + D, v at + 2 D
    float* stage = lds;
    float* sc = lds + AT_STAGE + wave * 16 * SP;
    const int q0 = (blockIdx.x * (nthr >> 6) + wave) * 16;
    const bool active = q0 < T;          // wave-uniform; an inactive wavefront still stages and keeps the barriers

    float qf[16];
    {
        const int q = q0 + li;
#pragma unroll
        for (int s = 0; s < 16; ++s) qf[s] = q < T ? base[q * row3 + 4 * s + lg] : 0.0f;
    }

    // ---- S = Q K^T * 0.125 into the score tile, 32 keys at a time
    for (int c0 = 0; c0 < Tc; c0 += AT_KC) {
        __syncthreads();
        for (int i = tid; i < AT_KC * (AT_HD / 2); i += nthr) {
            const int r = i >> 5, c2 = (i & 31) * 2, j = c0 + r;
            float2 v = make_float2(0.0f, 0.0f);
            if (j < T) v = *(const float2*)(base + D + j * row3 + c2);
            *(float2*)(stage + r * AT_KP + c2) = v;
        }
        __syncthreads();
        if (active) {
            f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
            const float* k0 = stage + li * AT_KP + lg;
            const float* k1 = k0 + 16 * AT_KP;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[s], k0[4 * s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[s], k1[4 * s], acc1, 0, 0, 0);
            }
            float* o = sc + (lg * 4) * SP + c0 + li;   // D: row (query) = 4 lg + e, column (key) = li
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e * SP] = acc0[e] * 0.125f;
                o[e * SP + 16] = acc1[e] * 0.125f;
            }
        }
    }
    __syncthreads();

    // ---- softmax of the wavefront's 16 rows, 4 lanes per row
    if (active) {
        float* row = sc + (lane >> 2) * SP;
        const int sub = lane & 3;
        float m = -INFINITY;
        for (int j = sub; j < T; j += 4) m = fmaxf(m, row[j]);
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        float c = 0.0f;
        for (int j = sub; j < T; j += 4) {
            const float e = dm_exp(row[j] - m);
            row[j] = e;
            c = c + e;
        }
        c = c + __shfl_xor(c, 1);
        c = c + __shfl_xor(c, 2);
        for (int j = sub; j < T; j += 4) row[j] = dm_div(row[j], c);
        for (int j = T + sub; j < Tc; j += 4) row[j] = 0.0f;
    }

    // ---- O = P V, 32 keys at a time (the barrier in front of the first chunk also orders the p writes above before the operand reads)
    f32x4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0, o2 = o0, o3 = o0;
    for (int c0 = 0; c0 < Tc; c0 += AT_KC) {
        __syncthreads();
        for (int i = tid; i < AT_KC * (AT_HD / 4); i += nthr) {
            const int r = i >> 4, c4 = (i & 15) * 4, j = c0 + r;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (j < T) v = *(const float4*)(base + 2 * D + j * row3 + c4);
            *(float4*)(stage + r * AT_VP + c4) = v;
        }
        __syncthreads();
        if (active) {
            const float* p = sc + li * SP + c0 + lg;
            const float* v = stage + lg * AT_VP + li;
#pragma unroll
            for (int s = 0; s < AT_KC / 4; ++s) {
                const float a = p[4 * s];
                const float* vs = v + 4 * s * AT_VP;
                o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vs[0], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vs[16], o1, 0, 0, 0);
                o2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vs[32], o2, 0, 0, 0);
                o3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vs[48], o3, 0, 0, 0);
            }
        }
    }
    if (!active) return;
    float* ob = out + (int64_t)n * T * D + h * AT_HD + li;   // D: row (query) = 4 lg + e, column (d within a 16-wide tile) = li
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = q0 + lg * 4 + e;
        if (q < T) {
            float* o = ob + (int64_t)q * D;
            o[0] = o0[e]; o[16] = o1[e]; o[32] = o2[e]; o[48] = o3[e];
        }
    }
}

__global__ void __launch_bounds__(256) vit_layer_norm_kernel(const float* x, int64_t rows, int D, int64_t x_stride, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * x_stride;
    const int nslot = D >> 2;
    const float K = xr[0];
    float4 v[LN_MAX_SLOTS];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < LN_MAX_SLOTS; ++k) {
        const int s = lane + 64 * k;
        if (s < nslot) {
            float4 t = *(const float4*)(xr + 4 * s);
            t.x = t.x - K; t.y = t.y - K; t.z = t.z - K; t.w = t.w - K;
            s1 = s1 + t.x; s2 = s2 + t.x * t.x;
            s1 = s1 + t.y; s2 = s2 + t.y * t.y;
            s1 = s1 + t.z; s2 = s2 + t.z * t.z;
            s1 = s1 + t.w; s2 = s2 + t.w * t.w;
            v[k] = t;
        }
    }
    double S1 = (double)s1, S2 = (double)s2;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        S1 = S1 + __shfl_xor(S1, off);
        S2 = S2 + __shfl_xor(S2, off);
    }
    const double md = S1 / (double)D;
    double var = S2 / (double)D - md * md;
    var = var > 0.0 ? var : 0.0;
    const float m = (float)md;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    float* orow = out + row * out_stride;
#pragma unroll
    for (int k = 0; k < LN_MAX_SLOTS; ++k) {
        const int s = lane + 64 * k;
        if (s < nslot) {
            const float4 ga = *(const float4*)(gamma + 4 * s), be = *(const float4*)(beta + 4 * s);
            float4 y;
            y.x = ((v[k].x - m) * rstd) * ga.x + be.x;
            y.y = ((v[k].y - m) * rstd) * ga.y + be.y;
            y.z = ((v[k].z - m) * rstd) * ga.z + be.z;
            y.w = ((v[k].w - m) * rstd) * ga.w + be.w;
            *(float4*)(orow + 4 * s) = y;
        }
    }
}

template <int TANH>
__device__ __forceinline__ float gelu1(float x) {
    float t;
    if (TANH) {
        const float x3 = (x * x) * x;
        t = dm_tanh(0.7978845608028654f * (x + 0.044715f * x3));
    } else {
        t = dm_erf(x * 0.7071067811865476f);
    }
    return (0.5f * x) * (1.0f + t);
}

template <int TANH>
__global__ void __launch_bounds__(256) vit_gelu_kernel(const float* x, float* y, int64_t n) {
    const int64_t n4 = n >> 2, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n4; i += step) {
        float4 v = ((const float4*)x)[i];
        v.x = gelu1<TANH>(v.x); v.y = gelu1<TANH>(v.y); v.z = gelu1<TANH>(v.z); v.w = gelu1<TANH>(v.w);
        ((float4*)y)[i] = v;
    }
    const int64_t i = n4 * 4 + t0;   // the tail of a length that is no multiple of 4
    if (i < n) y[i] = gelu1<TANH>(x[i]);
}

__global__ void __launch_bounds__(256) vit_patchify_kernel(const float* __restrict__ in, int H, int W, int P, int64_t total, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one output float
    if (i >= total) return;
    const int gw = W / P, gh = H / P, K = P * P * 3;
    const int k = (int)(i % K);
    const int64_t cell = i / K;
    const int gx = (int)(cell % gw), gy = (int)((cell / gw) % gh);
    const int64_t n = cell / ((int64_t)gw * gh);
    const int c = k % 3, px = (k / 3) % P, py = k / (3 * P);
    out[i] = in[((n * H + gy * P + py) * W + gx * P + px) * 3 + c];
}

__global__ void __launch_bounds__(64) vit_softmax_kernel(const float* __restrict__ x, int n, float* __restrict__ prob) {
    const int l = threadIdx.x;
    const float* xr = x + (int64_t)blockIdx.x * n;
    float* pr = prob + (int64_t)blockIdx.x * n;
    float m = -INFINITY;
    for (int j = l; j < n; j += 64) m = fmaxf(m, xr[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float c = 0.0f;
    for (int j = l; j < n; j += 64) {
        const float e = dm_exp(xr[j] - m);
        pr[j] = e;
        c = c + e;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c = c + __shfl_xor(c, off);
    for (int j = l; j < n; j += 64) pr[j] = dm_div(pr[j], c);
}

}  // namespace

int vit_attention_launch(const float* qkv, int N, int T, int heads, float* out, hipStream_t st) {
    ARG_CHECK(N >= 0 && T >= 1 && T <= 1024 && heads >= 1 && heads <= 65535, "attention: N >= 0, 1 <= T <= 1024, 1 <= heads (head dimension 64)");
    if (N == 0) return ISEGMI_OK;
    ARG_CHECK(N <= 65535, "attention: at most 65535 images");
    ARG_CHECK(qkv && out && qkv != out, "attention: null pointer (or out == qkv)");
    ARG_CHECK(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0, "attention: pointers must be 16-byte aligned");
    const int Tc = (T + AT_KC - 1) / AT_KC * AT_KC;
    int W = 4;
    if ((AT_STAGE + W * 16 * (Tc + 2)) * 4 > AT_LDS_MAX) W = 2;
    const int lds = (AT_STAGE + W * 16 * (Tc + 2)) * 4;
    LDS_LIMIT_ONCE(AT_LDS_MAX, vit_attention_kernel);
    hipLaunchKernelGGL(vit_attention_kernel, dim3((unsigned)cdiv(T, 16 * W), (unsigned)heads, (unsigned)N), dim3(64 * W), (size_t)lds, st, qkv, T, heads, Tc, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int vit_layer_norm_launch(const float* x, int64_t rows, int D, int64_t x_stride, const float* gamma, const float* beta, float eps, float* out,
                          int64_t out_stride, hipStream_t st) {
    ARG_CHECK(rows >= 0 && D >= 4 && D % 4 == 0 && D <= 256 * LN_MAX_SLOTS, "layer_norm: D must be a multiple of 4 in 4..2048");
    ARG_CHECK(x_stride >= D && out_stride >= D && x_stride % 4 == 0 && out_stride % 4 == 0, "layer_norm: row strides must be multiples of 4, at least D");
    ARG_CHECK(eps >= 0.0f, "layer_norm: eps must be a non-negative number");
    if (rows == 0) return ISEGMI_OK;
    ARG_CHECK(x && gamma && beta && out, "layer_norm: null pointer");
    ARG_CHECK(((uintptr_t)x | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "layer_norm: pointers must be 16-byte aligned");
    ARG_CHECK(rows <= 4ll * 0x7fffffff, "layer_norm: too many rows");
    hipLaunchKernelGGL(vit_layer_norm_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, st, x, rows, D, x_stride, gamma, beta, eps, out, out_stride);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int vit_gelu_launch(const float* x, float* y, int64_t n, int gelu_tanh, hipStream_t st) {
    ARG_CHECK(n >= 0 && (gelu_tanh == 0 || gelu_tanh == 1), "gelu: n >= 0, gelu_tanh 0 (erf) or 1 (tanh)");
    if (n == 0) return ISEGMI_OK;
    ARG_CHECK(x && y, "gelu: null pointer");
    ARG_CHECK(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "gelu: pointers must be 16-byte aligned");
    int64_t blocks = cdiv64(cdiv64(n, 4), 256);
    const int64_t cap = (int64_t)device_cu_count() * 16;
    if (blocks > cap) blocks = cap;
    if (gelu_tanh) hipLaunchKernelGGL(vit_gelu_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, x, y, n);
    else hipLaunchKernelGGL(vit_gelu_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, x, y, n);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int vit_patchify_launch(const float* in, int N, int H, int W, int P, float* out, hipStream_t st) {
    ARG_CHECK(N >= 0 && H > 0 && W > 0 && P > 0 && H % P == 0 && W % P == 0, "patchify: H and W must be positive multiples of P");
    const int64_t total = (int64_t)N * H * W * 3;
    if (total == 0) return ISEGMI_OK;
    ARG_CHECK(in && out && in != out, "patchify: null pointer (or out == in)");
    ARG_CHECK(cdiv64(total, 256) <= 0x7fffffff, "patchify: too many pixels");
    hipLaunchKernelGGL(vit_patchify_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, in, H, W, P, total, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int vit_softmax_launch(const float* x, int rows, int n, float* prob, hipStream_t st) {
    ARG_CHECK(rows >= 0 && n >= 1, "class_softmax: rows >= 0, n >= 1");
    if (rows == 0) return ISEGMI_OK;
    ARG_CHECK(x && prob && x != prob, "class_softmax: null pointer (or prob == logits)");
    hipLaunchKernelGGL(vit_softmax_kernel, dim3((unsigned)rows), dim3(64), 0, st, x, n, prob);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_attention(const float* d_qkv, int N, int T, int heads, float* d_out, void* stream) {
    return vit_attention_launch(d_qkv, N, T, heads, d_out, (hipStream_t)stream);
}
extern "C" int isegmi_op_layer_norm(const float* d_x, int64_t rows, int D, int64_t x_row_stride, const float* d_gamma, const float* d_beta, float eps,
                                    float* d_out, int64_t out_row_stride, void* stream) {
    return vit_layer_norm_launch(d_x, rows, D, x_row_stride, d_gamma, d_beta, eps, d_out, out_row_stride, (hipStream_t)stream);
}
extern "C" int isegmi_op_gelu(const float* d_x, float* d_y, int64_t n, int gelu_tanh, void* stream) {
    return vit_gelu_launch(d_x, d_y, n, gelu_tanh, (hipStream_t)stream);
}
extern "C" int isegmi_op_patchify(const float* d_in_nhwc3, int N, int H, int W, int P, float* d_out, void* stream) {
    return vit_patchify_launch(d_in_nhwc3, N, H, W, P, d_out, (hipStream_t)stream);
}
extern "C" int isegmi_op_class_softmax(const float* d_logits, int rows, int n, float* d_prob, void* stream) {
    return vit_softmax_launch(d_logits, rows, n, d_prob, (hipStream_t)stream);
}
