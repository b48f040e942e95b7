// bbox_aug.hip -- test-time box augmentation (TEST.BBOX_AUG): the per-view candidate stage.
//
// A view's raw box-predictor output (class logits + box regressions of the N x R proposals) becomes candidates of the per-image POOL, in the first
// view's coordinates: for every live proposal row r and class j >= 1 with p = softmax(logits[r])[j] > score_thresh (strict), the box
// clip(decode(props[r], deltas[r, j])) -- unflipped when the view is mirrored, then scaled to view 0 -- is appended behind what the views before left
// there, in (proposal asc, class asc) order.  The merge is isegmi_op_retina_postprocess over the pool (nseg 1, seg_len cap): no second NMS is written.
//
// Two launches per view for all N images, no atomics, bitwise reproducible:
//   count : one wave per row (softmax_row_wave, the plain tail's arithmetic), ballots over the classes -> the row's candidate count, max and sum
//           (12 bytes per row; no probability tensor is written).  Row 0 of every image snapshots the pool count the view starts from.
//   place : one block per 16 rows.  The block sums the image's row counts (those in front of its rows = its offset; all of them = the view's
//           total, which block 0 adds to the pool's counters), then every wave recomputes p = exp(x - max) / sum for its rows -- the same two
//           roundings on the same inputs, so the same bits and the same decisions as the count -- and writes score, label and box at
//           offset + ballot rank.  The logits are read from HBM once: the second launch finds the image's 324 KB (1000 x 81) in L2.
// A slot at or past `cap` is not written; d_pool_total keeps counting, so total > cap is the overflow signal and the pool holds the first cap candidates.
#include "../../include/isegmi.h"
#include "common.h"
#include "tail_launch.h"
#include "detbox.h"
#include "detsoftmax.h"

namespace isegmi {

constexpr int AUG_ROWS = 16;          // rows per block of the place kernel (4 per wave)
constexpr int AUG_MAX_R = 1024, AUG_MAX_CLS = 256, AUG_MAX_CAP = 8192;

struct AugK {
    int N, R, C, agnostic, hflip, cap;
    float thr;
    int64_t ls, rs;
    const float* logits; const float* regr; const float* props; const int* prop_cnt; const int* image_hw; const float* ratios;
    int* rowcnt; float* rowmax; float* rowsum; int* base;   // workspace: [N][R] x 3, [N]
    float* pool_boxes; float* pool_scores; int* pool_labels; int* pool_cnt; int* pool_total;
};

__device__ __forceinline__ int aug_live_rows(const AugK& a, int n) {
    const int c = a.prop_cnt[n];
    return c < 0 ? 0 : (c > a.R ? a.R : c);
}

// grid ceil(N * R / 4), 256 threads: wave = row
__global__ __launch_bounds__(256) void bbox_aug_count_kernel(const AugK a) {
    __shared__ float ex[4][SOFTMAX_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 4 + wave;
    if (g >= (int64_t)a.N * a.R) return;   // whole wave; no block barrier below
    const int n = (int)(g / a.R), r = (int)(g % a.R);
    int cnt = 0;
    float m = 0.0f, sum = 1.0f;
    if (r < aug_live_rows(a, n)) {   // (uniform) rows at or past the count are never read
        float v[SOFTMAX_Q];
        sum = softmax_row_wave(a.logits + g * a.ls, a.C, lane, ex[wave], v, &m);
#pragma unroll
        for (int q = 0; q < SOFTMAX_Q; ++q) {
            const int c = lane + 64 * q;
            const bool ok = c >= 1 && c < a.C && softmax_prob(v[q], sum) > a.thr;
            cnt += __popcll(__ballot(ok));
        }
    }
    if (lane == 0) {
        a.rowcnt[g] = cnt; a.rowmax[g] = m; a.rowsum[g] = sum;
        if (r == 0) {   // the slot this view's first candidate goes to
            const int b = a.pool_cnt[n];
            a.base[n] = b < 0 ? 0 : (b > a.cap ? a.cap : b);
        }
    }
}

// grid (ceil(R / AUG_ROWS), N), 256 threads
__global__ __launch_bounds__(256) void bbox_aug_place_kernel(const AugK a) {
    __shared__ int part[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, row0 = blockIdx.x * AUG_ROWS;
    const int* rc = a.rowcnt + (int64_t)n * a.R;
    int before = 0, all = 0;   // integer sums: order-free
    for (int i = tid; i < a.R; i += 256) {
        const int c = rc[i];
        all += c;
        before += i < row0 ? c : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { before += __shfl_xor(before, off, 64); all += __shfl_xor(all, off, 64); }
    if (lane == 0) { part[0][wave] = before; part[1][wave] = all; }
    __syncthreads();
    before = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    all = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    const int base = a.base[n];
    if (blockIdx.x == 0 && tid == 0) {   // the only writer of the counters; every reader of this launch takes the snapshot `base`
        a.pool_cnt[n] = base + all < a.cap ? base + all : a.cap;
        a.pool_total[n] = a.pool_total[n] + all;
    }
    const int myc = (lane < AUG_ROWS && row0 + lane < a.R) ? rc[row0 + lane] : 0;
    const float im_h = (float)a.image_hw[2 * n], im_w = (float)a.image_hw[2 * n + 1];
    const float rw = a.ratios[2 * n], rh = a.ratios[2 * n + 1];
    int run = base + before;
    for (int k = 0; k < AUG_ROWS; ++k) {
        const int ck = __shfl(myc, k, 64);
        if ((k & 3) == wave && ck > 0 && run < a.cap) {   // (uniform) ck > 0: a live row
            const int64_t g = (int64_t)n * a.R + row0 + k;
            const float m = a.rowmax[g], sum = a.rowsum[g];
            const float* lg = a.logits + g * a.ls;
            const float4 pr = *(const float4*)(a.props + g * 4);
            int pos = run;
#pragma unroll
            for (int q = 0; q < SOFTMAX_Q; ++q) {
                const int c = lane + 64 * q;
                float p = 0.0f;
                bool ok = false;
                if (c >= 1 && c < a.C) { p = softmax_prob(softmax_exp(lg[c], m), sum); ok = p > a.thr; }
                const unsigned long long bm = __ballot(ok);
                const int slot = pos + __popcll(bm & ((1ull << lane) - 1ull));
                if (ok && slot < a.cap) {
                    // CLS_AGNOSTIC_BBOX_REG: rows of eight, every class decodes the last four (as box_cls_nms_kernel)
                    const float* dp = a.regr + g * a.rs + (a.agnostic ? 4 : 4 * c);
                    float4 b = clip_box(decode_box(pr, make_float4(dp[0], dp[1], dp[2], dp[3]), 10.f, 10.f, 5.f, 5.f), im_w, im_h);
                    if (a.hflip) {   // BoxList.transpose(FLIP_LEFT_RIGHT), TO_REMOVE = 1: after the clip, in the view's own width
                        const float x1 = (im_w - b.z) - 1.0f, x2 = (im_w - b.x) - 1.0f;
                        b.x = x1; b.z = x2;
                    }
                    b.x = b.x * rw; b.y = b.y * rh; b.z = b.z * rw; b.w = b.w * rh;   // BoxList.resize to view 0
                    const int64_t o = (int64_t)n * a.cap + slot;
                    *(float4*)(a.pool_boxes + o * 4) = b;
                    a.pool_scores[o] = p;
                    a.pool_labels[o] = c;
                }
                pos += __popcll(bm);
            }
        }
        run += ck;
    }
}

static inline int64_t aug_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int64_t bbox_aug_workspace_bytes(int N, int R) {
    if (N < 1 || R < 1 || R > AUG_MAX_R) return -1;
    return 3 * aug_align256((int64_t)N * R * 4) + aug_align256((int64_t)N * 4);
}

int bbox_aug_candidates_launch(const BBoxAugArgs* p, hipStream_t st) {
    ARG_CHECK(p->N >= 1 && p->R >= 1 && p->R <= AUG_MAX_R, "bbox_aug_candidates: N >= 1, 1 <= R <= 1024");
    ARG_CHECK(p->ncls >= 2 && p->ncls <= AUG_MAX_CLS, "bbox_aug_candidates: 2 <= ncls <= 256");
    ARG_CHECK(p->cap >= 1 && p->cap <= AUG_MAX_CAP, "bbox_aug_candidates: 1 <= cap <= 8192");
    ARG_CHECK(p->logits_stride >= p->ncls && p->regr_stride >= (p->cls_agnostic ? 8 : 4 * (int64_t)p->ncls), "bbox_aug_candidates: row strides shorter than a row");
    ARG_CHECK(p->d_logits && p->d_regr && p->d_props && p->d_prop_cnt && p->d_image_hw && p->d_ratios_wh && p->d_ws && p->d_pool_boxes && p->d_pool_scores &&
              p->d_pool_labels && p->d_pool_cnt && p->d_pool_total, "bbox_aug_candidates: null device pointer");
    const int64_t need = bbox_aug_workspace_bytes(p->N, p->R);
    ARG_CHECK(p->ws_bytes >= need, "bbox_aug_candidates: workspace too small (isegmi_op_bbox_aug_workspace)");
    AugK a;
    a.N = p->N; a.R = p->R; a.C = p->ncls; a.agnostic = p->cls_agnostic ? 1 : 0; a.hflip = p->hflip ? 1 : 0; a.cap = p->cap;
    a.thr = p->score_thresh; a.ls = p->logits_stride; a.rs = p->regr_stride;
    a.logits = p->d_logits; a.regr = p->d_regr; a.props = p->d_props; a.prop_cnt = p->d_prop_cnt; a.image_hw = p->d_image_hw; a.ratios = p->d_ratios_wh;
    char* w = (char*)p->d_ws;
    const int64_t rows = aug_align256((int64_t)p->N * p->R * 4);
    a.rowcnt = (int*)w; w += rows;
    a.rowmax = (float*)w; w += rows;
    a.rowsum = (float*)w; w += rows;
    a.base = (int*)w;
    a.pool_boxes = p->d_pool_boxes; a.pool_scores = p->d_pool_scores; a.pool_labels = p->d_pool_labels; a.pool_cnt = p->d_pool_cnt; a.pool_total = p->d_pool_total;
    hipLaunchKernelGGL(bbox_aug_count_kernel, dim3((unsigned)cdiv64((int64_t)p->N * p->R, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(bbox_aug_place_kernel, dim3((unsigned)cdiv(p->R, AUG_ROWS), (unsigned)p->N), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int64_t isegmi_op_bbox_aug_workspace(int N, int R) { return bbox_aug_workspace_bytes(N, R); }
extern "C" int isegmi_op_bbox_aug_candidates(int N, int R, int ncls, int cls_agnostic, int hflip, int cap, float score_thresh, const float* d_logits,
                                             int64_t logits_stride, const float* d_regr, int64_t regr_stride, const float* d_props, const int32_t* d_prop_cnt,
                                             const int32_t* d_image_hw, const float* d_ratios_wh, void* d_ws, int64_t ws_bytes, float* d_pool_boxes,
                                             float* d_pool_scores, int32_t* d_pool_labels, int32_t* d_pool_cnt, int32_t* d_pool_total, void* stream) {
    BBoxAugArgs a;
    a.N = N; a.R = R; a.ncls = ncls; a.cls_agnostic = cls_agnostic; a.hflip = hflip; a.cap = cap; a.score_thresh = score_thresh;
    a.logits_stride = logits_stride; a.regr_stride = regr_stride; a.ws_bytes = ws_bytes;
    a.d_logits = d_logits; a.d_regr = d_regr; a.d_props = d_props; a.d_ratios_wh = d_ratios_wh; a.d_prop_cnt = d_prop_cnt; a.d_image_hw = d_image_hw;
    a.d_ws = d_ws; a.d_pool_boxes = d_pool_boxes; a.d_pool_scores = d_pool_scores; a.d_pool_labels = d_pool_labels; a.d_pool_cnt = d_pool_cnt;
    a.d_pool_total = d_pool_total;
    return bbox_aug_candidates_launch(&a, (hipStream_t)stream);
}
