// cocoeval.hip -- the device half of COCO evaluation: mask IoU straight on run-length encodings, box IoU,
// object keypoint similarity (OKS), and the greedy detection <-> ground-truth matching of COCOeval.evaluateImg.  Everything that describes
// pycocotools (maskApi.c rleArea / rleToBbox / rleIou / bbIou, cocoeval.py computeOks / evaluateImg) is [UPSTREAM-RECALL -- unverified]:
// restated from memory, upstream source is not available.
//
//   coco_rle_prefix   one block per RLE: inclusive prefix sums of its run counts -> run END positions (bounds) and the number of set pixels up
//                     to and including each run (cum); from them the area (rleArea) and the tight box (rleToBbox) of the mask
//   coco_rle_iou      one wave per (det, gt) pair: each lane takes 1-runs [s, e) of the side with fewer runs and binary-searches the other side's
//                     bounds for F(e) - F(s), F(p) = set pixels before position p; the integer partial sums are added across the wave with
//                     shuffles.  Intersection and areas are integers (exact, order-independent); the one floating operation is one IEEE double division
//   coco_bbox_iou     one thread per pair, bbIou's operation order
//   coco_oks          one thread per pair: computeOks' operation order, the terms added in keypoint-index order
//   coco_match        one thread per (group, area range, IoU threshold): the sequential greedy scan
//
// No atomics, no LDS beyond the block scans of coco_rle_prefix, nothing allocated here.
#include "../../include/isegmi.h"
#include "common.h"

namespace isegmi {

// ---------------------------------------------------------------------------------------------------------------- prefix / area / box
// grid (M), 256 threads.  counts[off[m] .. off[m + 1]) are the runs of RLE m (column-major, zeros first); hw[m] = (h, w).
// bounds[i] = counts[0] + .. + counts[i] (the END of run i; run i covers [bounds[i - 1], bounds[i])), cum[i] = set pixels in runs 0 .. i.
// bbox[m] = (x0, y0, x1, y1) inclusive, (0, 0, -1, -1) for an empty mask.  A 1-run of zero length is skipped (upstream's rleToBbox does not
// special-case it; rleEncode never produces one).
__global__ __launch_bounds__(256) void coco_rle_prefix_kernel(const uint32_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ hw, uint32_t* __restrict__ bounds,
                                                              uint32_t* __restrict__ cum, int64_t* __restrict__ area, int32_t* __restrict__ bbox) {
    __shared__ uint32_t wsum[2][4];
    __shared__ int red[4][4];
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t b = off[m], n = off[m + 1] - b;
    const uint32_t h = hw[2 * m] > 0 ? (uint32_t)hw[2 * m] : 1u;
    uint32_t carry_pos = 0, carry_set = 0;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (int64_t i0 = 0; i0 < n; i0 += 256) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t c = i < n ? counts[b + i] : 0u;
        const uint32_t s = (i & 1) ? c : 0u;
        uint32_t ic = c, is = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t oc = __shfl_up(ic, d, 64), os = __shfl_up(is, d, 64);
            if (lane >= d) { ic += oc; is += os; }
        }
        if (lane == 63) { wsum[0][wv] = ic; wsum[1][wv] = is; }
        __syncthreads();
        uint32_t base_c = 0, base_s = 0, tot_c = 0, tot_s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = wsum[0][k], q = wsum[1][k];
            if (k < wv) { base_c += a; base_s += q; }
            tot_c += a; tot_s += q;
        }
        const uint32_t end = carry_pos + base_c + ic;
        if (i < n) {
            bounds[b + i] = end;
            cum[b + i] = carry_set + base_s + is;
            if ((i & 1) && c > 0u) {
                const uint32_t first = end - c, last = end - 1u;
                const int xs = (int)(first / h), xe = (int)(last / h);
                const int ys = (int)(first - (uint32_t)xs * h), ye = (int)(last - (uint32_t)xe * h);
                xmin = xs < xmin ? xs : xmin;
                xmax = xe > xmax ? xe : xmax;
                if (xs < xe) { ymin = 0; ymax = (int)h - 1; }   // the run wraps into the next column: every row is touched
                else { ymin = ys < ymin ? ys : ymin; ymax = ye > ymax ? ye : ymax; }
            }
        }
        carry_pos += tot_c; carry_set += tot_s;
        __syncthreads();   // wsum is rewritten by the next round
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_down(xmin, d, 64), q = __shfl_down(ymin, d, 64), r = __shfl_down(xmax, d, 64), t = __shfl_down(ymax, d, 64);
        xmin = a < xmin ? a : xmin; ymin = q < ymin ? q : ymin; xmax = r > xmax ? r : xmax; ymax = t > ymax ? t : ymax;
    }
    if (lane == 0) { red[0][wv] = xmin; red[1][wv] = ymin; red[2][wv] = xmax; red[3][wv] = ymax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            xmin = red[0][k] < xmin ? red[0][k] : xmin; ymin = red[1][k] < ymin ? red[1][k] : ymin;
            xmax = red[2][k] > xmax ? red[2][k] : xmax; ymax = red[3][k] > ymax ? red[3][k] : ymax;
        }
        area[m] = (int64_t)carry_set;
        const bool empty = xmax < 0;
        bbox[4 * m + 0] = empty ? 0 : xmin; bbox[4 * m + 1] = empty ? 0 : ymin;
        bbox[4 * m + 2] = empty ? -1 : xmax; bbox[4 * m + 3] = empty ? -1 : ymax;
    }
}

// ---------------------------------------------------------------------------------------------------------------- mask IoU
// F(p): set pixels of the RLE (bounds, cum, n runs) at positions < p.  Run i covers [bounds[i - 1], bounds[i]); the run that holds p is the
// first one whose end lies beyond p (zero-length runs are stepped over by the same test).
__device__ __forceinline__ uint32_t coco_set_before(const uint32_t* __restrict__ bnd, const uint32_t* __restrict__ cum, int64_t n, uint32_t p) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (bnd[mid] > p) hi = mid; else lo = mid + 1;
    }
    if (lo == n) return n > 0 ? cum[n - 1] : 0u;
    uint32_t before = lo > 0 ? cum[lo - 1] : 0u;
    if (lo & 1) before += p - bnd[lo - 1];   // lo is odd, so lo - 1 >= 0
    return before;
}

// grid (ceil(P / 4)), 256 threads = 4 waves = 4 pairs.  pairs[p] = (det rle, gt rle, crowd).  out[p] = inter / union, inter / area(det) for a
// crowd gt, exactly 0.0 when inter == 0 (disjoint tight boxes are answered without a search); -1.0 flags a pair the caller must not have
// sent: an index outside [0, M) or two RLEs of different sizes.
__global__ __launch_bounds__(256) void coco_rle_iou_kernel(const uint32_t* __restrict__ bounds, const uint32_t* __restrict__ cum,
                                                           const int64_t* __restrict__ off, const int32_t* __restrict__ hw,
                                                           const int64_t* __restrict__ area, const int32_t* __restrict__ bbox, int M,
                                                           const int32_t* __restrict__ pairs, int64_t P, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;   // wave-uniform
    const int d = pairs[3 * p], g = pairs[3 * p + 1];
    const bool crowd = pairs[3 * p + 2] != 0;
    if (d < 0 || d >= M || g < 0 || g >= M || hw[2 * d] != hw[2 * g] || hw[2 * d + 1] != hw[2 * g + 1]) {
        if (lane == 0) out[p] = -1.0;
        return;
    }
    const int32_t* bd = bbox + 4 * (int64_t)d;
    const int32_t* bg = bbox + 4 * (int64_t)g;
    // an empty mask has x1 < x0, which makes it disjoint from everything
    if (bd[2] < bd[0] || bg[2] < bg[0] || bd[2] < bg[0] || bg[2] < bd[0] || bd[3] < bg[1] || bg[3] < bd[1]) {
        if (lane == 0) out[p] = 0.0;
        return;
    }
    int64_t oa = off[d], na = off[d + 1] - oa, ob = off[g], nb = off[g + 1] - ob;
    if (nb < na) { int64_t t = oa; oa = ob; ob = t; t = na; na = nb; nb = t; }   // walk the side with fewer runs, search the other (inter is symmetric)
    const uint32_t* bndA = bounds + oa;
    const uint32_t* bndB = bounds + ob;
    const uint32_t* cumB = cum + ob;
    unsigned long long inter = 0;
    for (int64_t j = lane; j < (na >> 1); j += 64) {
        const uint32_t s = bndA[2 * j], e = bndA[2 * j + 1];   // run 2j + 1 is a 1-run: [s, e)
        if (e > s) inter += (unsigned long long)(coco_set_before(bndB, cumB, nb, e) - coco_set_before(bndB, cumB, nb, s));
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) inter += __shfl_down(inter, k, 64);
    if (lane == 0) {
        const unsigned long long ad = (unsigned long long)area[d], ag = (unsigned long long)area[g];
        const unsigned long long u = crowd ? ad : ad + ag - inter;
        out[p] = inter == 0ull ? 0.0 : (double)inter / (double)u;
    }
}

// ---------------------------------------------------------------------------------------------------------------- box IoU
// bbIou's order, every operation one IEEE double operation (the library is built with -ffp-contract=off):
//   da = dw * dh; ga = gw * gh
//   w = min(dx + dw, gx + gw) - max(dx, gx); w <= 0 -> 0.0;  h = min(dy + dh, gy + gh) - max(dy, gy); h <= 0 -> 0.0
//   i = w * h;  u = crowd ? da : (da + ga) - i;  o = i / u
__global__ __launch_bounds__(256) void coco_bbox_iou_kernel(const double* __restrict__ boxes, int B, const int32_t* __restrict__ pairs, int64_t P,
                                                            double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int d = pairs[3 * p], g = pairs[3 * p + 1];
    const bool crowd = pairs[3 * p + 2] != 0;
    if (d < 0 || d >= B || g < 0 || g >= B) { out[p] = -1.0; return; }
    const double* D = boxes + 4 * (int64_t)d;
    const double* G = boxes + 4 * (int64_t)g;
    const double dx = D[0], dy = D[1], dw = D[2], dh = D[3], gx = G[0], gy = G[1], gw = G[2], gh = G[3];
    const double da = dw * dh, ga = gw * gh;
    const double xr = fmin(dx + dw, gx + gw), xl = fmax(dx, gx);
    const double w = xr - xl;
    double o = 0.0;
    if (w > 0.0) {
        const double yb = fmin(dy + dh, gy + gh), yt = fmax(dy, gy);
        const double h = yb - yt;
        if (h > 0.0) {
            const double i = w * h;
            const double u = crowd ? da : (da + ga) - i;
            o = i / u;
        }
    }
    out[p] = o;
}

// ---------------------------------------------------------------------------------------------------------------- keypoint similarity (OKS)
// [UPSTREAM-RECALL -- unverified] COCOeval.computeOks, every operation one IEEE double operation in this order (-ffp-contract=off):
//   k1 = #{k : vg_k > 0}
//   k1 > 0 : only the keypoints with vg_k > 0 count;  dx = xd - xg, dy = yd - yg
//   k1 == 0: all K count;  x0 = bx - bw, x1 = bx + bw * 2, dx = max(0, x0 - xd) + max(0, xd - x1), y likewise (the gt's coordinates are not read)
//   e = ((dx * dx + dy * dy) / vars_k) / (area + 2^-52) / 2;   oks = (exp(-e_0) + exp(-e_1) + ..) / n,  n = k1, or K when k1 == 0
// The terms are added in keypoint-index order, one add each (upstream's np.sum pairs them differently: a stated deviation).  A
// keypoint that does not count is branched over, never multiplied by zero: its coordinates may hold anything, NaN included.  The det's v is not read.
// One thread per pair, the whole sum in that thread: the value of a pair depends on nothing but its two items.  The pairs of a group are a
// row-major [D][G] block, so the lanes of a wave hold a few detections against the same G gts: one load instruction touches at most G distinct gt
// records and ceil(64 / G) + 1 det records, the rest of the lanes read an address another lane reads.  -1.0 flags an index outside [0, M).
__global__ __launch_bounds__(256) void coco_oks_kernel(const double* __restrict__ kpts, const double* __restrict__ box,
                                                       const double* __restrict__ area, const double* __restrict__ vars, int M, int K,
                                                       const int32_t* __restrict__ pairs, int64_t P, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int d = pairs[3 * p], g = pairs[3 * p + 1];
    if (d < 0 || d >= M || g < 0 || g >= M) { out[p] = -1.0; return; }
    const double* kd = kpts + (int64_t)d * K * 3;
    const double* kg = kpts + (int64_t)g * K * 3;
    int k1 = 0;
    for (int k = 0; k < K; ++k) k1 += kg[3 * k + 2] > 0.0 ? 1 : 0;
    const double den = area[g] + 0x1p-52;   // np.spacing(1)
    double sum = 0.0;
    if (k1 > 0) {
        for (int k = 0; k < K; ++k) {
            if (!(kg[3 * k + 2] > 0.0)) continue;
            const double dx = kd[3 * k] - kg[3 * k], dy = kd[3 * k + 1] - kg[3 * k + 1];
            const double e = (dx * dx + dy * dy) / vars[k] / den / 2.0;
            sum = sum + exp(-e);
        }
    } else {
        const double* b = box + 4 * (int64_t)g;
        const double x0 = b[0] - b[2], x1 = b[0] + b[2] * 2.0, y0 = b[1] - b[3], y1 = b[1] + b[3] * 2.0;
        for (int k = 0; k < K; ++k) {
            const double xd = kd[3 * k], yd = kd[3 * k + 1];
            const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
            const double e = (dx * dx + dy * dy) / vars[k] / den / 2.0;
            sum = sum + exp(-e);
        }
    }
    out[p] = sum / (double)(k1 > 0 ? k1 : K);
}

// ---------------------------------------------------------------------------------------------------------------- greedy matching
struct CocoMatchK {
    int n_groups, A, T;
    int64_t n_dets, n_gts, n_ious;
    const int64_t *det_off, *gt_off, *iou_off;
    const double *ious, *det_area, *gt_area, *area_rng, *iou_thrs;
    const uint8_t *gt_crowd, *gt_ignore;
    int32_t *dt_match, *gt_match;
    uint8_t *dt_ignore, *gt_ignore_out;
};

// one thread per (group, area range a, threshold t), t fastest: the T threads of one (group, a) read the same IoU block.
// The gt_match slice [a][t][group's gts] doubles as the scan's "already matched" flags: it is cleared here first.
__global__ __launch_bounds__(256) void coco_match_kernel(const CocoMatchK p) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)p.n_groups * p.A * p.T) return;
    const int t = (int)(id % p.T);
    const int a = (int)((id / p.T) % p.A);
    const int grp = (int)(id / ((int64_t)p.T * p.A));
    const int64_t d0 = p.det_off[grp], d1 = p.det_off[grp + 1], g0 = p.gt_off[grp], g1 = p.gt_off[grp + 1];
    if (d0 < 0 || d1 < d0 || d1 > p.n_dets || g0 < 0 || g1 < g0 || g1 > p.n_gts) return;   // malformed offsets: touch nothing
    const int64_t D = d1 - d0, G = g1 - g0, io = p.iou_off[grp];
    const bool have_iou = D > 0 && G > 0;
    if (have_iou && (io < 0 || io + D * G > p.n_ious)) return;
    const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
    const double thr = fmin(p.iou_thrs[t], 1.0 - 1e-10);
    const int64_t at = (int64_t)a * p.T + t;
    int32_t* dtm = p.dt_match + at * p.n_dets + d0;
    uint8_t* dti = p.dt_ignore + at * p.n_dets + d0;
    int32_t* gtm = p.gt_match + at * p.n_gts + g0;
    const double* ga = p.gt_area + g0;
    const uint8_t* gc = p.gt_crowd + g0;
    const uint8_t* gi = p.gt_ignore + g0;
#define COCO_GT_IG(k) (gi[k] != 0 || gc[k] != 0 || ga[k] < lo || ga[k] > hi)
    for (int64_t k = 0; k < G; ++k) {
        gtm[k] = 0;
        if (t == 0) p.gt_ignore_out[(int64_t)a * p.n_gts + g0 + k] = COCO_GT_IG(k) ? 1 : 0;
    }
    for (int64_t d = 0; d < D; ++d) {
        double best = thr;
        int64_t m = -1;
        const double* row = p.ious + io + d * G;
        // gts in stable order, non-ignored first: pass 0 visits the non-ignored ones; the ignored ones (pass 1) are only reached while no
        // match is held, because a held match at that point is a non-ignored one and the scan stops at the first ignored gt after it
        for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass) {
            for (int64_t k = 0; k < G; ++k) {
                if ((COCO_GT_IG(k) ? 1 : 0) != pass) continue;
                if (gtm[k] > 0 && gc[k] == 0) continue;
                if (row[k] < best) continue;
                best = row[k];
                m = k;
            }
        }
        uint8_t ig;
        if (m >= 0) {
            ig = COCO_GT_IG(m) ? 1 : 0;
            gtm[m] = (int32_t)(d + 1);
        } else {
            const double da = p.det_area[d0 + d];
            ig = (da < lo || da > hi) ? 1 : 0;
        }
        dtm[d] = (int32_t)(m + 1);
        dti[d] = ig;
    }
#undef COCO_GT_IG
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_coco_rle_prefix_bytes(int64_t total_runs, int M, int64_t* bounds_bytes, int64_t* cum_bytes, int64_t* area_bytes,
                                            int64_t* bbox_bytes) {
    ARG_CHECK(total_runs >= 0 && M >= 0, "rle_prefix sizes");
    if (bounds_bytes) *bounds_bytes = total_runs * 4;
    if (cum_bytes) *cum_bytes = total_runs * 4;
    if (area_bytes) *area_bytes = (int64_t)M * 8;
    if (bbox_bytes) *bbox_bytes = (int64_t)M * 16;
    return ISEGMI_OK;
}

extern "C" int isegmi_op_rle_prefix(const uint32_t* d_counts, const int64_t* d_off, const int32_t* d_hw, int M, uint32_t* d_bounds,
                                    uint32_t* d_cum, int64_t* d_area, int32_t* d_bbox, void* stream) {
    ARG_CHECK(M >= 0, "rle_prefix: M");
    if (M == 0) return ISEGMI_OK;
    ARG_CHECK(d_counts && d_off && d_hw && d_bounds && d_cum && d_area && d_bbox, "rle_prefix: null pointer");
    hipLaunchKernelGGL(coco_rle_prefix_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, d_counts, d_off, d_hw, d_bounds, d_cum,
                       d_area, d_bbox);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_rle_iou(const uint32_t* d_bounds, const uint32_t* d_cum, const int64_t* d_off, const int32_t* d_hw,
                                 const int64_t* d_area, const int32_t* d_bbox, int M, const int32_t* d_pairs, int64_t P, double* d_out,
                                 void* stream) {
    ARG_CHECK(M >= 0 && P >= 0 && P < (1ll << 32), "rle_iou sizes");
    if (P == 0) return ISEGMI_OK;
    ARG_CHECK(d_bounds && d_cum && d_off && d_hw && d_area && d_bbox && d_pairs && d_out, "rle_iou: null pointer");
    hipLaunchKernelGGL(coco_rle_iou_kernel, dim3((unsigned)cdiv64(P, 4)), dim3(256), 0, (hipStream_t)stream, d_bounds, d_cum, d_off, d_hw,
                       d_area, d_bbox, M, d_pairs, P, d_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_bbox_iou(const double* d_boxes, int B, const int32_t* d_pairs, int64_t P, double* d_out, void* stream) {
    ARG_CHECK(B >= 0 && P >= 0 && P < (1ll << 38), "bbox_iou sizes");
    if (P == 0) return ISEGMI_OK;
    ARG_CHECK(d_boxes && d_pairs && d_out, "bbox_iou: null pointer");
    hipLaunchKernelGGL(coco_bbox_iou_kernel, dim3((unsigned)cdiv64(P, 256)), dim3(256), 0, (hipStream_t)stream, d_boxes, B, d_pairs, P, d_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_oks(const double* d_kpts, const double* d_box, const double* d_area, const double* d_vars, int M, int K,
                             const int32_t* d_pairs, int64_t P, double* d_out, void* stream) {
    ARG_CHECK(M >= 0 && K >= 1 && K <= 32 && P >= 0 && P < (1ll << 38), "oks sizes");
    if (P == 0) return ISEGMI_OK;
    ARG_CHECK(d_kpts && d_box && d_area && d_vars && d_pairs && d_out, "oks: null pointer");
    hipLaunchKernelGGL(coco_oks_kernel, dim3((unsigned)cdiv64(P, 256)), dim3(256), 0, (hipStream_t)stream, d_kpts, d_box, d_area, d_vars, M, K,
                       d_pairs, P, d_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_coco_match_bytes(int64_t n_dets, int64_t n_gts, int A, int T, int64_t* dt_match_bytes, int64_t* dt_ignore_bytes,
                                       int64_t* gt_match_bytes, int64_t* gt_ignore_bytes) {
    ARG_CHECK(n_dets >= 0 && n_gts >= 0 && A > 0 && T > 0, "coco_match sizes");
    if (dt_match_bytes) *dt_match_bytes = (int64_t)A * T * n_dets * 4;
    if (dt_ignore_bytes) *dt_ignore_bytes = (int64_t)A * T * n_dets;
    if (gt_match_bytes) *gt_match_bytes = (int64_t)A * T * n_gts * 4;
    if (gt_ignore_bytes) *gt_ignore_bytes = (int64_t)A * n_gts;
    return ISEGMI_OK;
}

extern "C" int isegmi_op_coco_match(const isegmi_coco_match_args* a, void* stream) {
    ARG_CHECK(a, "coco_match: null args");
    ARG_CHECK(a->n_groups >= 0 && a->A > 0 && a->T > 0 && a->n_dets >= 0 && a->n_gts >= 0 && a->n_ious >= 0, "coco_match sizes");
    if (a->n_groups == 0) return ISEGMI_OK;
    ARG_CHECK(a->d_det_off && a->d_gt_off && a->d_iou_off && a->d_area_rng && a->d_iou_thrs, "coco_match: null table");
    ARG_CHECK(a->n_ious == 0 || a->d_ious, "coco_match: null ious");
    ARG_CHECK(a->n_dets == 0 || (a->d_det_area && a->d_dt_match && a->d_dt_ignore), "coco_match: null det array");
    ARG_CHECK(a->n_gts == 0 || (a->d_gt_area && a->d_gt_crowd && a->d_gt_ignore && a->d_gt_match && a->d_gt_ignore_out), "coco_match: null gt array");
    const int64_t threads = (int64_t)a->n_groups * a->A * a->T;
    ARG_CHECK(cdiv64(threads, 256) < (1ll << 31), "coco_match: too many scans for one launch");
    CocoMatchK p;
    p.n_groups = a->n_groups; p.A = a->A; p.T = a->T; p.n_dets = a->n_dets; p.n_gts = a->n_gts; p.n_ious = a->n_ious;
    p.det_off = a->d_det_off; p.gt_off = a->d_gt_off; p.iou_off = a->d_iou_off; p.ious = a->d_ious; p.det_area = a->d_det_area;
    p.gt_area = a->d_gt_area; p.area_rng = a->d_area_rng; p.iou_thrs = a->d_iou_thrs; p.gt_crowd = a->d_gt_crowd; p.gt_ignore = a->d_gt_ignore;
    p.dt_match = a->d_dt_match; p.gt_match = a->d_gt_match; p.dt_ignore = a->d_dt_ignore; p.gt_ignore_out = a->d_gt_ignore_out;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)cdiv64(threads, 256)), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}
