// yolact_coeff.hip -- mask coefficients of SELECTED priors (Yolact "lazy_coeffs").
//
// The fused prediction head (prediction_layers.0.head_cat) produces, per pixel of P3..P7, A x (4 loc + 81 conf + 32 mask coefficients).  Detect needs
// loc and conf of every prior, but the coefficients only of the <= max_num_detections priors per image that survive fast-NMS (upstream gathers
// mask_data[idx] after NMS, too).  So the forward runs the loc|conf rows of the head only, and the two kernels here supply the coefficient rows:
//
//   coeff_index : slot (n, q) of the final top-k -> its row (image, level, ho, wo, anchor), or -1s past the image's count
//   coeff_rows  : for every valid slot the 32 outputs of weight rows row0 + 32 a + j at that pixel of the level's upfeature map
//
// Numerics: each output is the convolution's accumulator chain restated -- acc = fmaf(x_k, w_k, acc) from +0 in the K order of conv_korder.h (the order
// the MFMA kernels walk; an fp32 MFMA is bit for bit such a chain), a padding tap contributing fmaf(0, w, acc) like the hardware-zeroed loads there, and
// the act 0 epilogue fmaf(acc, scale-or-1, shift-or-0) + 0.0f.  Pre-tanh, as the convolution stores them; the gather applies dm_tanh.
#include "../../include/isegmi.h"
#include "common.h"
#include "conv_korder.h"
#include "engine.h"

namespace isegmi {

constexpr int COEFF_ROW_INTS = 5;   // (image, level, ho, wo, anchor)

// grid (N); block 128: one thread per slot, as the gather
__global__ void yolact_coeff_index_kernel(const int* __restrict__ fin_idx, const int* __restrict__ tk_idx, const int* __restrict__ fin_cnt, int nc,
                                          int top_k, int max_det, int A, const CoeffLevels lv, int* __restrict__ rows) {
    const int n = blockIdx.x;
    const int cnt = fin_cnt[n];
    for (int q = threadIdx.x; q < max_det; q += blockDim.x) {
        int* r = rows + ((int64_t)n * max_det + q) * COEFF_ROW_INTS;
        int level = -1, ho = -1, wo = -1, a = -1;
        if (q < cnt) {
            const int prior = tk_idx[(int64_t)n * nc * top_k + fin_idx[(int64_t)n * max_det + q]];
            int pix = prior / A;
            a = prior - pix * A;
            for (int l = 0; l < lv.n; ++l) {
                const int hw = lv.H[l] * lv.W[l];
                if (pix < hw) { level = l; ho = pix / lv.W[l]; wo = pix - ho * lv.W[l]; break; }
                pix -= hw;
            }
        }
        r[0] = level < 0 ? -1 : n; r[1] = level; r[2] = ho; r[3] = wo; r[4] = a;
    }
}

// One wave per slot.  A first version -- one thread per output reading its own weight row from global memory, chunk by chunk -- was bound by the latency
// of its loads (72 dependent round trips of 64 scattered 16-byte loads: 83 us alone on the chip, 230 us under the next step's convolutions, where it took
// back half of what the narrower head gained; profiles/lazy_coeffs.md).  Here the 64 lanes fetch a STAGE -- up to four consecutive chunks of the walk, which
// lie side by side in the packed rows and in the input pixel -- of all 32 weight rows with coalesced 16-byte loads (a row's 512 bytes by 32 lanes) into
// registers while lanes 0..31 run the previous stage's fmaf chain from LDS, where a lane reads its own row (pitch 132 floats: conflict-free b128 reads)
// and the pixel's values as broadcasts.
constexpr int COEFF_STAGE_CHUNKS = 4, COEFF_WPITCH = COEFF_STAGE_CHUNKS * 32 + 4;
__global__ __launch_bounds__(64) void yolact_coeff_rows_kernel(const CoeffLevels lv, int N, int Cin, int R, int S, int pad, const float* __restrict__ w,
                                                                const float* __restrict__ scale, const float* __restrict__ shift, int A, int row0,
                                                                const int* __restrict__ rows, const int* __restrict__ count, int max_det,
                                                                float* __restrict__ out) {
    constexpr int MD = kYolactMaskDim;   // 32 outputs = 32 weight rows per slot
    __shared__ __attribute__((aligned(16))) float sw[2][MD * COEFF_WPITCH];
    __shared__ __attribute__((aligned(16))) float sx[2][COEFF_STAGE_CHUNKS * 32];
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int q = slot % max_det;
    if (q >= count[slot / max_det]) return;   // slots past the image's count are not written (block-uniform, like every return below)
    const int* r = rows + (int64_t)slot * COEFF_ROW_INTS;
    const int n = r[0], l = r[1], ho = r[2], wo = r[3], a = r[4];
    if (l < 0 || l >= lv.n || n < 0 || n >= N || a < 0 || a >= A) return;   // marked invalid
    const int H = lv.H[l], W = lv.W[l];
    if (ho < 0 || ho >= H || wo < 0 || wo >= W) return;
    const float* x = lv.feat[l] + (int64_t)n * H * W * Cin;
    const int cin_chunks = Cin / 32;
    const int64_t wrow = (int64_t)R * S * Cin;   // packed row: R * S * Cin floats, (r, s, cin) chunks
    const float* wr = w + (int64_t)(row0 + MD * a) * wrow;
    const int kgroup = conv_kgroup(R, S, cin_chunks, false);
    int kr = 0, ks = 0, kc = 0, kg = 0, glen = kgroup;   // walk position of the next stage to load
    int left = R * S * cin_chunks;                        // chunks not loaded yet
    typedef float4 StageRegs[4 * COEFF_STAGE_CHUNKS];
    // the next stage: nc <= 4 chunks of the current (tap, channel group) run, loaded into registers; the walk moves on by nc chunks
    auto load_stage = [&](StageRegs& rw, float4& rx) -> int {
        const int run = glen - kc;
        const int nc = run < COEFF_STAGE_CHUNKS ? run : COEFF_STAGE_CHUNKS;
        const int hi = ho - pad + kr, wi = wo - pad + ks;
        const bool ok = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
        const float* wp = wr + (int64_t)conv_k_wchunk(kr, ks, kc, kg, S, cin_chunks) * 32;
        // load i: rows 2 i and 2 i + 1, a lane per float4 of a row's (up to) 128 floats; in a short stage (nc < 4) the lanes past its end re-read float4 0
        const int c4 = (lane & 31) < 8 * nc ? (lane & 31) : 0;
        const float* wl = wp + (int64_t)(lane >> 5) * wrow + c4 * 4;
#pragma unroll
        for (int i = 0; i < 4 * COEFF_STAGE_CHUNKS; ++i) rw[i] = *(const float4*)(wl + (int64_t)(2 * i) * wrow);
        // a padding tap is a loaded 0, not a skipped product
        rx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok && lane < 8 * nc) rx = *(const float4*)(x + ((int64_t)hi * W + wi) * Cin + (kg + kc) * 32 + lane * 4);
        for (int i = 0; i < nc; ++i) (void)conv_k_next(kr, ks, kc, kg, glen, R, S, kgroup, cin_chunks);
        left -= nc;
        return nc;
    };
    auto store_stage = [&](const StageRegs& rw, const float4& rx, int buf, int nc) {
        if ((lane & 31) < 8 * nc) {
            float* d = &sw[buf][(lane >> 5) * COEFF_WPITCH + (lane & 31) * 4];
#pragma unroll
            for (int i = 0; i < 4 * COEFF_STAGE_CHUNKS; ++i) *(float4*)(d + 2 * i * COEFF_WPITCH) = rw[i];
        }
        if (lane < 8 * nc) *(float4*)(&sx[buf][lane * 4]) = rx;
    };
    float acc = 0.0f;
    int cur = 0;
    int nc_cur;
    {
        StageRegs rw;
        float4 rx;
        nc_cur = load_stage(rw, rx);
        store_stage(rw, rx, 0, nc_cur);
    }
    __syncthreads();
    while (true) {
        const bool more = left > 0;   // uniform
        StageRegs rw;   // the next stage travels in registers under this stage's chain
        float4 rx;
        const int nc_next = load_stage(rw, rx);   // (past the last stage the walk has wrapped to the row's first chunk: a harmless load, never stored)
        if (lane < MD) {
            const float* wl = &sw[cur][lane * COEFF_WPITCH];
            const float* xl = sx[cur];
            for (int g = 0; g < 4 * nc_cur; ++g) {   // 8-groups of the stage, k ascending
                const float4 x0 = *(const float4*)(xl + g * 8), x1 = *(const float4*)(xl + g * 8 + 4);
                const float4 w0 = *(const float4*)(wl + g * 8), w1 = *(const float4*)(wl + g * 8 + 4);
                const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf(xv[e], wv[conv_perm8(e)], acc);
            }
        }
        if (!more) break;
        store_stage(rw, rx, cur ^ 1, nc_next);   // the other buffer: its last readers finished an iteration ago
        __syncthreads();
        cur ^= 1;
        nc_cur = nc_next;
    }
    if (lane < MD) {
        const int co = row0 + MD * a + lane;
        const float sc = scale ? scale[co] : 1.0f, sh = shift ? shift[co] : 0.0f;
        out[(int64_t)slot * MD + lane] = fmaf(acc, sc, sh) + 0.0f;
    }
}

static int check_levels(const CoeffLevels& lv) {
    ARG_CHECK(lv.n >= 1 && lv.n <= 5, "1..5 feature levels");
    for (int l = 0; l < lv.n; ++l) ARG_CHECK(lv.feat[l] != nullptr && lv.H[l] > 0 && lv.W[l] > 0, "feature level");
    return ISEGMI_OK;
}

int yolact_coeff_index_launch(const int32_t* fin_idx, const int32_t* tk_idx, const int32_t* fin_cnt, int N, int nc, int top_k, int max_det, int A,
                              const CoeffLevels& lv, int32_t* rows, hipStream_t st) {
    ARG_CHECK(fin_idx && tk_idx && fin_cnt && rows && N > 0 && nc > 0 && top_k > 0 && max_det > 0 && A > 0, "coeff index args");
    TRY(check_levels(lv));
    hipLaunchKernelGGL(yolact_coeff_index_kernel, dim3(N), dim3(128), 0, st, fin_idx, tk_idx, fin_cnt, nc, top_k, max_det, A, lv, rows);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int yolact_coeff_rows_launch(const CoeffLevels& lv, int N, int Cin, int R, int S, int pad, const float* w_packed, const float* scale, const float* shift,
                             int A, int row0, int mask_dim, const int32_t* rows, const int32_t* count, int max_det, float* out, hipStream_t st) {
    ARG_CHECK(w_packed && rows && count && out && N > 0 && max_det > 0 && A > 0 && row0 >= 0 && mask_dim > 0, "coeff rows args");
    ARG_CHECK(Cin > 0 && Cin % 32 == 0 && R > 0 && S > 0 && pad >= 0, "coeff rows: Cin % 32 == 0, a stride-1 R x S kernel");
    TRY(check_levels(lv));
    ARG_CHECK(mask_dim == kYolactMaskDim, "coeff rows: mask_dim must be 32");
    ARG_CHECK((int64_t)N * max_det < (1ll << 31), "coeff rows: too many slots");
    hipLaunchKernelGGL(yolact_coeff_rows_kernel, dim3((unsigned)(N * max_det)), dim3(64), 0, st, lv, N, Cin, R, S, pad, w_packed, scale, shift, A, row0,
                       rows, count, max_det, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_yolact_coeff_rows(int nlevels, const float* const* d_feats, const int32_t* Hs, const int32_t* Ws, int N, int Cin, int R, int S,
                                           int pad, const float* d_wpacked, const float* d_scale, const float* d_shift, int A, int row0,
                                           const int32_t* d_rows, const int32_t* d_count, int max_det, float* d_out, void* stream) {
    ARG_CHECK(d_feats && Hs && Ws && nlevels >= 1 && nlevels <= 5 && A > 0, "coeff rows: levels");
    CoeffLevels lv;
    lv.n = nlevels;
    for (int l = 0; l < nlevels; ++l) { lv.feat[l] = d_feats[l]; lv.H[l] = Hs[l]; lv.W[l] = Ws[l]; }
    for (int l = nlevels; l < 5; ++l) { lv.feat[l] = nullptr; lv.H[l] = lv.W[l] = 0; }
    return yolact_coeff_rows_launch(lv, N, Cin, R, S, pad, d_wpacked, d_scale, d_shift, A, row0, kYolactMaskDim, d_rows, d_count, max_det, d_out,
                                    (hipStream_t)stream);
}
