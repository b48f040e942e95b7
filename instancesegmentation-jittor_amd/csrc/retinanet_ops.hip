// retinanet_ops.hip -- the RetinaNet inference tail: thresholded top-k selection over the class logits of all pyramid levels with the
// box decode fused into its last stage (retina_select), and class-wise NMS + the detections-per-image cut over the survivors (retina_postprocess).
//
// retina_select.  Rows are (level, image); a row is the cls_logits output of one image as the convolution wrote it, H*W*A*C floats, flat index
// ((y*W + x)*A + a)*C + c.  Two launches for all levels:
//   1. one block per (row, slice of RETINA_SLICE logits): the slice is read from HBM ONCE into LDS as sort keys -- f2ord(dm_sigmoid(x)) where the
//      sigmoid exceeds the threshold, 0 elsewhere -- so neither the sigmoid tensor nor a transposed copy ever exists.  A slice with more than top_n
//      candidates keeps its top_n best by a radix select over the 64-bit keys (score << 32 | ~index), which are unique: `key >= T` holds for exactly
//      top_n of them, ties at the cut going to the lower index.  The survivors leave in index order (ballot ranks, no atomics).
//   2. one block per row: the same select over the row's slice lists (any number of candidates, from none to every logit), a bitonic sort of the
//      <= 1024 winners by (score desc, index asc), then the decode of the selected: deltas and anchor gathered through the flat index,
//      BoxCoder(10, 10, 5, 5), clip to the unpadded image, min-size test, ordered compaction.
// The winners of launch 2 are appended to LDS through an atomic counter; the list holds exactly k_eff <= 1024 unique keys and is fully sorted
// afterwards, so nothing depends on arrival order.  Key order contract: csrc/detbox.h's, on the SIGMOID values (two logits may share one).
//
// retina_postprocess.  Per image up to 8192 candidate slots (nseg lists of seg_len, the first seg_cnt of each valid):
//   1. sort by (class asc, score desc, slot asc) in LDS; gather boxes / scores / labels in that order; class segment bounds;
//   2. suppression bitmask over the whole chip, only for 64 x 64 tiles whose rows and columns share a class; a bit needs equal labels, so a box
//      never suppresses a box of another class and no coordinate offset enters the IoU;
//   3. greedy scan, one wave per (image, class): a chunk of 64 is resolved from its diagonal word, kept rows OR their words into the removed set;
//   4. k-th value cut (scores >= the det_per_img-th largest kept score), output in class order -- NMS order inside a class, slot order under
//      ISEGMI_NMS_INDEX_ORDER -- at most cap rows.
#include "../../include/isegmi.h"
#include "common.h"
#include "detbox.h"
#include "tail_launch.h"
#include <float.h>
#include <math.h>

namespace isegmi {

namespace {

constexpr int RETINA_SLICE = 8192;      // logits per slice: 32 KB of keys in LDS
constexpr int RETINA_KCAP = 1024;       // top_n the kernels hold
constexpr int RETINA_NT = 1024;
constexpr int RETINA_BINS = DET_RADIX_BINS;
constexpr int RETINA_MAX_SLOTS = 8192;  // candidate slots per image in retina_postprocess: 64 KB of sort keys in LDS

struct RetinaLevel {
    const float* logits;   // [N][n]
    const float* deltas;   // [N][n / C][4]
    const float* anchors;  // [n / C][4]
    int n;                 // logits per row
    int slices;
    int blk0;              // first block of the level in launch 1
    int64_t cand0;         // first (row, slice) list of the level in the workspace
};
struct RetinaSelect {
    int nl, N, C, top_n;
    float thr, prefilter, min_size;
    RetinaLevel lv[ISEGMI_RETINA_MAX_LEVELS];
    unsigned long long* cand;   // [lists][top_n]
    int* cand_cnt;              // [lists]
    const int* image_hw;
    float* sel_scores; int* sel_idx; int* sel_cnt;
    float* out_boxes; float* out_scores; int* out_labels; int* out_cnt;
};

// launch 1: grid = sum over levels of N * slices
__global__ __launch_bounds__(RETINA_NT) void retina_slice_kernel(const RetinaSelect a) {
    __shared__ unsigned keys[RETINA_SLICE];
    __shared__ unsigned hist[RETINA_BINS];
    __shared__ unsigned sel[2];
    __shared__ unsigned wcnt[RETINA_NT / 64];
    constexpr int NW = RETINA_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int l = 0;
    while (l + 1 < a.nl && (int)blockIdx.x >= a.lv[l + 1].blk0) ++l;   // uniform
    const RetinaLevel& L = a.lv[l];
    const int b = (int)blockIdx.x - L.blk0;
    const int row = b / L.slices, slice = b - row * L.slices;
    const int off = slice * RETINA_SLICE;
    const int n = L.n - off < RETINA_SLICE ? L.n - off : RETINA_SLICE;
    const float* x = L.logits + (int64_t)row * L.n + off;

    // the slice's only trip to HBM: eight independent loads per thread
    unsigned mine = 0u;
#pragma unroll
    for (int q = 0; q < RETINA_SLICE / RETINA_NT; ++q) {
        const int i = tid + q * RETINA_NT;
        const float v = i < n ? x[i] : 0.0f;
        unsigned u = 0u;
        if (i < n && v >= a.prefilter) {   // >=: without a pre-filter (-inf) a -inf logit still reaches the sigmoid test; a NaN never passes either test
            const float p = dm_sigmoid(v);
            if (p > a.thr) u = f2ord(p);
        }
        keys[i] = u;
        mine += u != 0u;
    }
    mine += __shfl_xor(mine, 1, 64); mine += __shfl_xor(mine, 2, 64); mine += __shfl_xor(mine, 4, 64);
    mine += __shfl_xor(mine, 8, 64); mine += __shfl_xor(mine, 16, 64); mine += __shfl_xor(mine, 32, 64);
    if (lane == 0) wcnt[wave] = mine;
    __syncthreads();
    unsigned cnt = 0u;
    for (int w = 0; w < NW; ++w) cnt += wcnt[w];
    __syncthreads();
    const unsigned k_eff = cnt < (unsigned)a.top_n ? cnt : (unsigned)a.top_n;
    const int64_t list = L.cand0 + b;
    if (tid == 0) a.cand_cnt[list] = (int)k_eff;
    if (k_eff == 0u) return;
    auto key_of = [&](int i) { return det_key_ord(keys[i], off + i); };
    unsigned long long T = 1ull;
    if (cnt > k_eff)
        T = radix_select64([&](auto f) { for (int i = tid; i < n; i += RETINA_NT) if (keys[i] != 0u) f(key_of(i)); }, k_eff, hist, sel);

    // ordered compaction: wave w owns the contiguous keys [w * SEG, (w + 1) * SEG)
    constexpr int SEG = RETINA_SLICE / NW;
    const int s0 = wave * SEG;
    unsigned c = 0u;
    for (int i = s0 + lane; i < s0 + SEG; i += 64) c += __popcll(__ballot(keys[i] != 0u && key_of(i) >= T));
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    unsigned run = 0u;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long* out = a.cand + list * a.top_n;
    for (int i = s0 + lane; i < s0 + SEG; i += 64) {
        const unsigned long long k = key_of(i);
        const bool s = keys[i] != 0u && k >= T;
        const unsigned long long bm = __ballot(s);
        if (s) {
            const unsigned pos = run + (unsigned)__popcll(bm & lt);
            if (pos < k_eff) out[pos] = k;
        }
        run += (unsigned)__popcll(bm);
    }
}

// launch 2: grid = nl * N (block = level * N + image)
__global__ __launch_bounds__(RETINA_NT) void retina_merge_kernel(const RetinaSelect a) {
    __shared__ unsigned long long sbuf[RETINA_KCAP];
    __shared__ unsigned hist[RETINA_BINS];
    __shared__ unsigned sel[2];
    __shared__ unsigned wcnt[RETINA_NT / 64];
    __shared__ unsigned scount;
    constexpr int NW = RETINA_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = (int)blockIdx.x / a.N, img = (int)blockIdx.x - l * a.N;
    const RetinaLevel& L = a.lv[l];
    const int64_t list0 = L.cand0 + (int64_t)img * L.slices;
    const int* lcnt = a.cand_cnt + list0;
    const unsigned long long* cand = a.cand + list0 * a.top_n;

    unsigned mine = 0u;
    for (int s = tid; s < L.slices; s += RETINA_NT) mine += (unsigned)lcnt[s];
    mine += __shfl_xor(mine, 1, 64); mine += __shfl_xor(mine, 2, 64); mine += __shfl_xor(mine, 4, 64);
    mine += __shfl_xor(mine, 8, 64); mine += __shfl_xor(mine, 16, 64); mine += __shfl_xor(mine, 32, 64);
    if (lane == 0) wcnt[wave] = mine;
    if (tid == 0) scount = 0u;
    sbuf[tid] = 0ull;
    __syncthreads();
    unsigned total = 0u;
    for (int w = 0; w < NW; ++w) total += wcnt[w];
    __syncthreads();
    const unsigned k_eff = total < (unsigned)a.top_n ? total : (unsigned)a.top_n;
    auto each = [&](auto f) {   // wave w walks the slice lists w, w + NW, ...
        for (int s = wave; s < L.slices; s += NW) {
            const int c = lcnt[s];
            for (int j = lane; j < c; j += 64) f(cand[(int64_t)s * a.top_n + j]);
        }
    };
    unsigned long long T = 1ull;
    if (total > k_eff) T = radix_select64(each, k_eff, hist, sel);
    each([&](unsigned long long key) {
        if (key >= T) {
            const unsigned pos = atomicAdd(&scount, 1u);   // exactly k_eff unique keys pass; the sort below fixes their order
            if (pos < (unsigned)RETINA_KCAP) sbuf[pos] = key;
        }
    });
    __syncthreads();
    bitonic_sort<true>(sbuf, RETINA_KCAP, RETINA_NT);
    const int64_t orow = (int64_t)img * a.nl + l;
    const bool real = (unsigned)tid < k_eff;
    const unsigned long long kx = sbuf[tid];
    const float score = real ? det_key_score(kx) : -1.0f;
    const int idx = real ? det_key_index(kx) : -1;
    if (tid < a.top_n) {
        a.sel_scores[orow * a.top_n + tid] = score;
        a.sel_idx[orow * a.top_n + tid] = idx;
    }
    if (tid == 0) a.sel_cnt[orow] = (int)k_eff;
    if (a.out_boxes == nullptr) return;   // uniform: selection only

    // decode of the selected, in selection order
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    bool ok = false;
    if (real) {
        const int anchor = idx / a.C;
        const float4 an = *(const float4*)(L.anchors + (int64_t)anchor * 4);
        const float4 d = *(const float4*)(L.deltas + ((int64_t)img * (L.n / a.C) + anchor) * 4);
        box = clip_box(decode_box(an, d, 10.0f, 10.0f, 5.0f, 5.0f), (float)a.image_hw[img * 2 + 1], (float)a.image_hw[img * 2]);
        ok = box_min_size_ok(box, a.min_size);
    }
    const unsigned long long bm = __ballot(ok);
    if (lane == 0) wcnt[wave] = (unsigned)__popcll(bm);
    __syncthreads();
    unsigned run = 0u, tot = 0u;
    for (int w = 0; w < NW; ++w) { if (w < wave) run += wcnt[w]; tot += wcnt[w]; }
    const int64_t obase = orow * a.top_n;   // [N][nl * top_n]: level l's list starts at l * top_n
    if (ok) {
        const int64_t o = obase + run + (unsigned)__popcll(bm & ((1ull << lane) - 1ull));
        *(float4*)(a.out_boxes + o * 4) = box;
        a.out_scores[o] = score;
        a.out_labels[o] = idx % a.C + 1;
    }
    if (tid >= (int)tot && tid < a.top_n) {
        const int64_t o = obase + tid;
        *(float4*)(a.out_boxes + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        a.out_scores[o] = -1.0f;
        a.out_labels[o] = 0;
    }
    if (tid == 0) a.out_cnt[orow] = (int)tot;
}

// ------------------------------------------------------------------ retina_postprocess
struct RetinaPost {
    int N, nseg, seg_len, M, MP, MW, nc, det, cap, flags;
    float thr;
    const float* boxes; const float* scores; const int* labels; const int* seg_cnt;
    float* sbox; float* sscore; int* slabel; int* sslot; unsigned char* kept; int* cbound; int* total; unsigned long long* matrix;
    int* out_cnt; float* out_boxes; float* out_scores; int* out_labels;
};
constexpr int RETINA_CB = 512;   // cbound row: [256] class starts, [256] class ends

// grid N.  key = label << 45 | ~ord(score) << 13 | slot, ascending: (class asc, score desc, slot asc)
__global__ __launch_bounds__(1024) void retina_sort_kernel(const RetinaPost a) {
    extern __shared__ unsigned long long skeys[];
    __shared__ int cb[RETINA_CB];
    __shared__ int stotal;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int P = next_pow2(a.M);
    if (tid == 0) stotal = 0;
    for (int i = tid; i < RETINA_CB; i += blockDim.x) cb[i] = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += blockDim.x) {
        unsigned long long key = ~0ull;
        if (i < a.M) {
            const int seg = i / a.seg_len, j = i - seg * a.seg_len;
            const int64_t src = (int64_t)n * a.M + i;
            const int lab = j < a.seg_cnt[n * a.nseg + seg] ? a.labels[src] : 0;
            if (lab >= 1 && lab <= a.nc) {
                key = ((unsigned long long)lab << 45) | ((unsigned long long)(~f2ord(a.scores[src])) << 13) | (unsigned long long)i;
                ++mine;
            }
        }
        skeys[i] = key;
    }
    if (mine) atomicAdd(&stotal, mine);   // a count
    __syncthreads();
    bitonic_sort<false>(skeys, P, blockDim.x);
    const int total = stotal;
    for (int i = tid; i < total; i += blockDim.x) {
        const unsigned long long key = skeys[i];
        const int slot = (int)(key & 8191ull), lab = (int)(key >> 45);
        const int64_t src = (int64_t)n * a.M + slot, dst = (int64_t)n * a.MP + i;
        *(float4*)(a.sbox + dst * 4) = *(const float4*)(a.boxes + src * 4);
        a.sscore[dst] = a.scores[src];
        a.slabel[dst] = lab;
        a.sslot[dst] = slot;
        if (i == 0 || (int)(skeys[i - 1] >> 45) != lab) cb[lab] = i;
        if (i == total - 1 || (int)(skeys[i + 1] >> 45) != lab) cb[256 + lab] = i + 1;
    }
    __syncthreads();
    for (int i = tid; i < RETINA_CB; i += blockDim.x) a.cbound[n * RETINA_CB + i] = cb[i];
    if (tid == 0) a.total[n] = total;
}

// grid (ceil(pairs / 4), N), 256 threads: wave (r, w), r <= w, owns rows 64r.. x columns 64w.. of the suppression matrix
__global__ __launch_bounds__(256) void retina_matrix_kernel(const RetinaPost a) {
    __shared__ float4 cols[4][64];
    __shared__ int clab[4][64];
    const int n = blockIdx.y;
    const int total = a.total[n];
    const int nwords = (total + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r, w;
    tri_pair(blockIdx.x * 4 + wave, r, w);   // wave-uniform
    if (w >= nwords) return;   // whole wave; no block-level barrier below
    const int* lab = a.slabel + (int64_t)n * a.MP;
    const int rlast = (r << 6) + 63 < total ? (r << 6) + 63 : total - 1;
    if (lab[rlast] < lab[w << 6]) return;   // sorted by class: the tile's rows and columns share none
    const IouThr T = make_iou_thr(a.thr, a.flags & ISEGMI_NMS_GE);
    const float one = nms_one(a.flags);
    const float4* sb = (const float4*)(a.sbox + (int64_t)n * a.MP * 4);
    const int i = (r << 6) + lane, jc = (w << 6) + lane;
    const float4 mine = sb[i < total ? i : 0];
    const int mylab = lab[i < total ? i : 0];
    clab[wave][lane] = jc < total ? lab[jc] : -1;   // a column past `total` matches no class
    nms_stage_cols(cols[wave], lane, sb[jc < total ? jc : 0]);
    const int* cl = clab[wave];
    const unsigned long long bits = nms_tile_word(mine, cols[wave], i, w, one, T, [cl, mylab](int, int b) { return cl[b] == mylab; });
    if (i < total) a.matrix[((int64_t)n * a.MP + i) * a.MW + w] = bits;
}

// grid (nc, N), 64 threads: the greedy scan of class blockIdx.x + 1.  rem: lane q holds the removed bits of words w0 + q and w0 + 64 + q.
__global__ __launch_bounds__(64) void retina_scan_kernel(const RetinaPost a) {
    const int n = blockIdx.y, c = blockIdx.x + 1, lane = threadIdx.x;
    const int s = a.cbound[n * RETINA_CB + c], e = a.cbound[n * RETINA_CB + 256 + c];
    if (e <= s) return;
    const int w0 = s >> 6, w1 = (e - 1) >> 6;
    const unsigned long long* M = a.matrix + (int64_t)n * a.MP * a.MW;
    unsigned char* kept = a.kept + (int64_t)n * a.MP;
    unsigned long long rem0 = 0ull, rem1 = 0ull;
    for (int cw = w0; cw <= w1; ++cw) {
        const int i = (cw << 6) + lane;
        const bool in = i >= s && i < e;
        const unsigned long long d = in ? M[(int64_t)i * a.MW + cw] : 0ull;
        const int rel = cw - w0;
        const unsigned long long rsrc = rel < 64 ? rem0 : rem1;
        const unsigned long long rc = __shfl(rsrc, rel & 63, 64);
        const unsigned long long alive = nms_resolve_chunk(~rc & __ballot(in), d);
        if (in) kept[i] = (unsigned char)((alive >> lane) & 1ull);
        if (cw == w1) break;
        const int wa = w0 + lane, wb = w0 + 64 + lane;
        const bool ha = wa > cw && wa <= w1, hb = wb > cw && wb <= w1;
        unsigned long long m = alive;   // uniform
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1ull;
            const int64_t row = (int64_t)((cw << 6) + b) * a.MW;
            if (ha) rem0 |= M[row + wa];
            if (hb) rem1 |= M[row + wb];
        }
    }
}

// grid N, 1024 threads
__global__ __launch_bounds__(1024) void retina_finalize_kernel(const RetinaPost a) {
    extern __shared__ unsigned long long skeys[];
    __shared__ int scnt[2];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int total = a.total[n];
    const int P = next_pow2(total);
    const unsigned char* kept = a.kept + (int64_t)n * a.MP;
    const float* sscore = a.sscore + (int64_t)n * a.MP;
    if (tid < 2) scnt[tid] = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += blockDim.x) {
        const int ii = i < total ? i : 0;
        const bool k = i < total && kept[ii];
        skeys[i] = k ? (unsigned long long)(~f2ord(sscore[ii])) : ~0ull;
        mine += k;
    }
    if (mine) atomicAdd(&scnt[0], mine);
    __syncthreads();
    const int nk = scnt[0];
    unsigned cut = 0u;   // ordered key of the lowest score that stays
    if (a.det > 0 && nk > a.det) {
        bitonic_sort<false>(skeys, P, blockDim.x);
        cut = ~(unsigned)skeys[a.det - 1];
        __syncthreads();
    }
    const bool by_slot = (a.flags & ISEGMI_NMS_INDEX_ORDER) != 0;
    mine = 0;
    for (int i = tid; i < P; i += blockDim.x) {
        const int ii = i < total ? i : 0;
        const bool k = i < total && kept[ii] && f2ord(sscore[ii]) >= cut;
        const unsigned ord = by_slot ? (unsigned)a.sslot[(int64_t)n * a.MP + ii] : (unsigned)i;
        skeys[i] = k ? ((unsigned long long)a.slabel[(int64_t)n * a.MP + ii] << 32) | ((unsigned long long)ord << 16) | (unsigned long long)i : ~0ull;
        mine += k;
    }
    if (mine) atomicAdd(&scnt[1], mine);
    __syncthreads();
    bitonic_sort<false>(skeys, P, blockDim.x);
    const int cnt = scnt[1] < a.cap ? scnt[1] : a.cap;
    for (int q = tid; q < a.cap; q += blockDim.x) {
        const int64_t o = (int64_t)n * a.cap + q;
        if (q < cnt) {
            const int64_t src = (int64_t)n * a.MP + (int)(skeys[q] & 0xffffull);
            *(float4*)(a.out_boxes + o * 4) = *(const float4*)(a.sbox + src * 4);
            a.out_scores[o] = a.sscore[src];
            a.out_labels[o] = a.slabel[src];
        } else {
            *(float4*)(a.out_boxes + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            a.out_scores[o] = 0.0f;
            a.out_labels[o] = 0;
        }
    }
    if (tid == 0) a.out_cnt[n] = cnt;
}

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

}  // namespace

int64_t retina_select_workspace_bytes(int nl, int N, const int* HW, int A, int C, int top_n) {
    if (nl < 1 || nl > ISEGMI_RETINA_MAX_LEVELS || N < 1 || A < 1 || C < 1 || top_n < 1 || top_n > RETINA_KCAP) return -1;
    int64_t lists = 0;
    for (int l = 0; l < nl; ++l) {
        const int64_t n = (int64_t)HW[l] * A * C;
        if (HW[l] < 1 || n > 0x7fffffff) return -1;
        lists += (int64_t)N * ((n + RETINA_SLICE - 1) / RETINA_SLICE);
    }
    return align256(lists * top_n * 8) + align256(lists * 4);
}

int retina_select_launch(const isegmi_retina_select_args* p, hipStream_t st) {
    ARG_CHECK(p->nl >= 1 && p->nl <= ISEGMI_RETINA_MAX_LEVELS, "retina_select: 1-5 levels");
    ARG_CHECK(p->N >= 1 && p->A >= 1 && p->C >= 1, "retina_select sizes");
    ARG_CHECK(p->top_n >= 1 && p->top_n <= RETINA_KCAP, "retina_select: top_n <= 1024");
    ARG_CHECK(p->d_sel_scores && p->d_sel_idx && p->d_sel_cnt && p->d_ws, "retina_select: null device pointer");
    const bool decode = p->d_out_boxes != nullptr;
    ARG_CHECK(!decode || (p->d_out_scores && p->d_out_labels && p->d_out_cnt && p->d_image_hw), "retina_select: decode outputs come together, with d_image_hw");
    const int64_t need = retina_select_workspace_bytes(p->nl, p->N, p->HW, p->A, p->C, p->top_n);
    ARG_CHECK(need > 0 && p->ws_bytes >= need, "retina_select: workspace too small (isegmi_op_retina_select_workspace) or a level over 2^31 logits");
    RetinaSelect a;
    a.nl = p->nl; a.N = p->N; a.C = p->C; a.top_n = p->top_n;
    a.thr = p->score_thresh; a.min_size = p->min_size;
    // a logit can pass only if its sigmoid can: x > logit(thr), with a margin far above dm_sigmoid's few-ulp error.  The selection itself compares dm_sigmoid(x),
    // which never reaches 0 (it floors at 4.156e-39, for -inf too): under a threshold below the normal floats every number may pass, so there is no pre-filter.
    a.prefilter = -INFINITY;
    if (p->score_thresh >= FLT_MIN && p->score_thresh < 1.0f) a.prefilter = logf(p->score_thresh / (1.0f - p->score_thresh)) - 0.25f;
    int blk = 0;
    int64_t lists = 0;
    for (int l = 0; l < p->nl; ++l) {
        ARG_CHECK(p->d_logits[l] && (!decode || (p->d_deltas[l] && p->d_anchors[l])), "retina_select: null level pointer");
        RetinaLevel& L = a.lv[l];
        L.logits = p->d_logits[l]; L.deltas = p->d_deltas[l]; L.anchors = p->d_anchors[l];
        L.n = p->HW[l] * p->A * p->C;
        L.slices = (L.n + RETINA_SLICE - 1) / RETINA_SLICE;
        L.blk0 = blk; L.cand0 = lists;
        blk += p->N * L.slices;
        lists += (int64_t)p->N * L.slices;
    }
    a.cand = (unsigned long long*)p->d_ws;
    a.cand_cnt = (int*)((char*)p->d_ws + align256(lists * p->top_n * 8));
    a.image_hw = p->d_image_hw;
    a.sel_scores = p->d_sel_scores; a.sel_idx = p->d_sel_idx; a.sel_cnt = p->d_sel_cnt;
    a.out_boxes = p->d_out_boxes; a.out_scores = p->d_out_scores; a.out_labels = p->d_out_labels; a.out_cnt = p->d_out_cnt;
    hipLaunchKernelGGL(retina_slice_kernel, dim3(blk), dim3(RETINA_NT), 0, st, a);
    hipLaunchKernelGGL(retina_merge_kernel, dim3(p->nl * p->N), dim3(RETINA_NT), 0, st, a);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int64_t retina_post_workspace_bytes(int N, int nseg, int seg_len) {
    const int64_t M = (int64_t)nseg * seg_len;
    if (N < 1 || nseg < 1 || seg_len < 1 || M > RETINA_MAX_SLOTS) return -1;
    const int64_t MP = (M + 63) & ~(int64_t)63, MW = MP / 64;
    return align256(N * MP * 16) + 3 * align256(N * MP * 4) + align256(N * MP) + align256((int64_t)N * RETINA_CB * 4) + align256(N * 4) + align256(N * MP * MW * 8);
}

int retina_postprocess_launch(const isegmi_retina_post_args* p, hipStream_t st) {
    ARG_CHECK(p->N >= 1 && p->nseg >= 1 && p->seg_len >= 1 && (int64_t)p->nseg * p->seg_len <= RETINA_MAX_SLOTS, "retina_postprocess: at most 8192 candidate slots per image");
    ARG_CHECK(p->ncls >= 2 && p->ncls <= 256, "retina_postprocess: 2 <= ncls <= 256");
    ARG_CHECK(p->cap >= 1 && p->det_per_img >= 0 && p->nms_thresh > 0.0f, "retina_postprocess: cap / det_per_img / nms_thresh");
    ARG_CHECK((p->nms_flags & ~7) == 0, "retina_postprocess: nms_flags is an OR of ISEGMI_NMS_*");
    ARG_CHECK(p->d_boxes && p->d_scores && p->d_labels && p->d_seg_cnt && p->d_ws && p->d_out_count && p->d_out_boxes && p->d_out_scores && p->d_out_labels,
              "retina_postprocess: null device pointer");
    const int64_t need = retina_post_workspace_bytes(p->N, p->nseg, p->seg_len);
    ARG_CHECK(p->ws_bytes >= need, "retina_postprocess: workspace too small (isegmi_op_retina_postprocess_workspace)");
    RetinaPost a;
    a.N = p->N; a.nseg = p->nseg; a.seg_len = p->seg_len; a.M = p->nseg * p->seg_len;
    a.MP = (a.M + 63) & ~63; a.MW = a.MP / 64;
    a.nc = p->ncls - 1; a.det = p->det_per_img; a.cap = p->cap; a.flags = p->nms_flags; a.thr = p->nms_thresh;
    a.boxes = p->d_boxes; a.scores = p->d_scores; a.labels = p->d_labels; a.seg_cnt = p->d_seg_cnt;
    char* w = (char*)p->d_ws;
    const int64_t N = p->N, MP = a.MP;
    a.sbox = (float*)w; w += align256(N * MP * 16);
    a.sscore = (float*)w; w += align256(N * MP * 4);
    a.slabel = (int*)w; w += align256(N * MP * 4);
    a.sslot = (int*)w; w += align256(N * MP * 4);
    a.kept = (unsigned char*)w; w += align256(N * MP);
    a.cbound = (int*)w; w += align256(N * RETINA_CB * 4);
    a.total = (int*)w; w += align256(N * 4);
    a.matrix = (unsigned long long*)w;
    a.out_cnt = p->d_out_count; a.out_boxes = p->d_out_boxes; a.out_scores = p->d_out_scores; a.out_labels = p->d_out_labels;
    const int P = next_pow2(a.M);
    const size_t lds = (size_t)P * 8;
    LDS_LIMIT_ONCE(RETINA_MAX_SLOTS * 8, retina_sort_kernel);
    LDS_LIMIT_ONCE(RETINA_MAX_SLOTS * 8, retina_finalize_kernel);
    hipLaunchKernelGGL(retina_sort_kernel, dim3(p->N), dim3(1024), lds, st, a);
    const int pairs = a.MW * (a.MW + 1) / 2;
    hipLaunchKernelGGL(retina_matrix_kernel, dim3((pairs + 3) / 4, p->N), dim3(256), 0, st, a);
    hipLaunchKernelGGL(retina_scan_kernel, dim3(a.nc, p->N), dim3(64), 0, st, a);
    hipLaunchKernelGGL(retina_finalize_kernel, dim3(p->N), dim3(1024), lds, st, a);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int64_t isegmi_op_retina_select_workspace(int nl, int N, const int32_t* HW, int A, int C, int top_n) {
    if (HW == nullptr) return -1;
    return retina_select_workspace_bytes(nl, N, HW, A, C, top_n);
}
extern "C" int isegmi_op_retina_select(const isegmi_retina_select_args* a, void* stream) {
    ARG_CHECK(a != nullptr, "null args");
    return retina_select_launch(a, (hipStream_t)stream);
}
extern "C" int64_t isegmi_op_retina_postprocess_workspace(int N, int nseg, int seg_len) { return retina_post_workspace_bytes(N, nseg, seg_len); }
extern "C" int isegmi_op_retina_postprocess(const isegmi_retina_post_args* a, void* stream) {
    ARG_CHECK(a != nullptr, "null args");
    return retina_postprocess_launch(a, (hipStream_t)stream);
}
