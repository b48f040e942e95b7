// yolo_ops.hip -- the YOLOv3 inference tail and the route of its heads ([UPSTREAM-RECALL] the public yolov3.cfg, unverified).
//
// yolo_select.  Rows are (level, image); a row is one image's head output as the convolution wrote it: H*W*A anchor records of REC = 5 + C floats
// (tx, ty, tw, th, to, C class logits).  A candidate is a (record, class) pair with flat index record * C + c = ((y*W + x)*A + a)*C + c and score
// s = obj * p_c, obj = dm_sigmoid(to), p_c = dm_sigmoid(t_c): one rounded fp32 multiply (the file is compiled with -ffp-contract=off).  Two launches for
// all levels, built like retina_select (csrc/retinanet_ops.hip) on the unique 64-bit keys of csrc/detbox.h:
//   1. one block per (row, slice of whole records, at most YOLO_SLICE floats): every head float of the slice is loaded from HBM ONCE, coalesced, into
//      registers.  The objectness logits go to LDS; one thread per record turns them into obj, or into 0 where !(obj > thr).  That test is an EXACT
//      pre-filter, not a heuristic: p = RN(1 / RN(1 + e)) with e >= 0 has a divisor >= 1, so p <= 1; then the real product obj * p <= obj, and rounding
//      to nearest is monotone and leaves the representable obj in place, so RN(obj * p) <= obj.  s > thr therefore implies obj > thr, and a record that
//      fails the test can hold no candidate (tests/test_yolov3_cpu.py samples the inequality over the float range).  Only the class logits of surviving
//      records reach the sigmoid.  Their keys f2ord(s) (0: no candidate) stand in LDS at record * C + c; multi_label 0 first stores f2ord(p) there and one
//      thread per record keeps the class of the largest sigmoid VALUE, lowest index on ties.  A slice with more than top_n candidates keeps its top_n
//      best by the radix select; survivors leave in index order (ballot ranks, no atomics); the slice's count BEFORE the cut is written as well.
//   2. one block per row: the same select over the row's slice lists (from none to every (anchor, class) pair), a bitonic sort of the <= 1024 winners by
//      (s desc, index asc), the row's pre-cut total, then the decode of the selected: tx..th gathered through the flat index (the only second read of
//      a head float: four per selected candidate), bx = (dm_sigmoid(tx) + x) * stride, bw = dm_exp(tw) * anchor_w, corners bx -+ bw * 0.5, clip to the
//      canvas, NaN and min_wh drop, ordered compaction into retina_postprocess's input layout.
// The winners of launch 2 are appended to LDS through an atomic counter; the list holds exactly k_eff unique keys and is fully sorted afterwards, so
// nothing depends on arrival order.
//
// concat_up2x.  out[n][y][x] = [coarse[n][y/2][x/2] (Cc) | skip[n][y][x] (Cs)]: darknet's upsample + route in one pass, one 16-byte access per thread.
#include "../../include/isegmi.h"
#include "common.h"
#include "detbox.h"
#include "tail_launch.h"
#include <string.h>

namespace isegmi {

namespace {

constexpr int YOLO_SLICE = 8192;   // head floats per slice, and the LDS key slots of a slice (a slice's C * records keys are fewer)
constexpr int YOLO_KCAP = 1024;    // top_n the kernels hold
constexpr int YOLO_NT = 1024;
constexpr int YOLO_MT = 512;     // threads of the merge launch
constexpr int YOLO_MAX_A = 8;
constexpr int YOLO_MAX_REC = YOLO_SLICE / 6;   // records of the narrowest record (C = 1)

struct YoloLevel {
    const float* head;   // [N][nrec][REC]
    int H, W, nrec;      // nrec = H * W * A
    int slices;
    int blk0;            // first block of the level in launch 1
    int64_t cand0;       // first (row, slice) list of the level in the workspace
    float stride;
    float aw[YOLO_MAX_A], ah[YOLO_MAX_A];
};
struct YoloSelect {
    int nl, N, A, C, top_n, rs, multi_label;   // rs: records per slice
    float thr, min_wh, canvas_w, canvas_h;
    YoloLevel lv[ISEGMI_YOLO_MAX_LEVELS];
    unsigned long long* cand;   // [lists][top_n]
    int* cand_cnt;              // [lists] after the slice's cut
    int* cand_tot;              // [lists] before it
    float* out_boxes; float* out_scores; int* out_labels; int* out_cnt; int* out_total;
};

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    return v;
}

// launch 1: grid = sum over levels of N * slices
__global__ __launch_bounds__(YOLO_NT) void yolo_slice_kernel(const YoloSelect a) {
    __shared__ unsigned keys[YOLO_SLICE];
    __shared__ float sobj[YOLO_MAX_REC];
    __shared__ unsigned hist[DET_RADIX_BINS];
    __shared__ unsigned sel[2];
    __shared__ unsigned wcnt[YOLO_NT / 64];
    constexpr int NW = YOLO_NT / 64, Q = YOLO_SLICE / YOLO_NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int l = 0;
    while (l + 1 < a.nl && (int)blockIdx.x >= a.lv[l + 1].blk0) ++l;   // uniform
    const YoloLevel& L = a.lv[l];
    const int b = (int)blockIdx.x - L.blk0;
    const int row = b / L.slices, slice = b - row * L.slices;
    const int C = a.C, REC = C + 5;
    const int rec0 = slice * a.rs;
    const int nrec = L.nrec - rec0 < a.rs ? L.nrec - rec0 : a.rs;
    const int nf = nrec * REC, nk = nrec * C;   // floats and key slots of this slice
    const float* x = L.head + ((int64_t)row * L.nrec + rec0) * REC;

    // the slice's only trip to HBM: eight independent coalesced loads per thread, kept in registers
    float v[Q];
    int rr[Q], kk[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = tid + q * YOLO_NT;
        v[q] = i < nf ? x[i] : 0.0f;
        rr[q] = i / REC;
        kk[q] = i - rr[q] * REC;
        if (i < nf && kk[q] == 4) sobj[rr[q]] = v[q];
    }
    __syncthreads();
    unsigned alive = 0u;
    for (int r = tid; r < nrec; r += YOLO_NT) {
        const float o = dm_sigmoid(sobj[r]);
        const bool pass = o > a.thr;   // NaN never passes
        sobj[r] = pass ? o : 0.0f;     // obj > 0 always: 0 marks a record without candidates
        alive += pass;
    }
    alive = wave_sum(alive);
    if (lane == 0) wcnt[wave] = alive;
    __syncthreads();
    unsigned nalive = 0u;
    for (int w = 0; w < NW; ++w) nalive += wcnt[w];
    __syncthreads();
    const int64_t list = L.cand0 + b;
    if (nalive == 0u) {   // uniform: the common slice of a trained model
        if (tid == 0) { a.cand_cnt[list] = 0; a.cand_tot[list] = 0; }
        return;
    }

    unsigned mine = 0u;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = tid + q * YOLO_NT;
        if (i < nf && kk[q] >= 5) {
            const float o = sobj[rr[q]];
            unsigned u = 0u;
            if (o != 0.0f) {
                const float p = dm_sigmoid(v[q]);
                if (a.multi_label) {
                    const float s = o * p;
                    if (s > a.thr) u = f2ord(s);
                } else {
                    u = f2ord(p);   // p > 0: never the empty key
                }
            }
            keys[rr[q] * C + kk[q] - 5] = u;
            mine += a.multi_label && u != 0u;
        }
    }
    if (!a.multi_label) {   // uniform
        __syncthreads();
        for (int r = tid; r < nrec; r += YOLO_NT) {
            const float o = sobj[r];
            if (o == 0.0f) continue;
            unsigned best = 0u;
            int bc = 0;
            for (int c = 0; c < C; ++c) {
                const unsigned u = keys[r * C + c];
                if (u > best) { best = u; bc = c; }   // strict: the lowest index of equal sigmoids stays
                keys[r * C + c] = 0u;
            }
            const float s = o * ord2f(best);
            if (s > a.thr) { keys[r * C + bc] = f2ord(s); ++mine; }
        }
    }
    mine = wave_sum(mine);
    if (lane == 0) wcnt[wave] = mine;
    __syncthreads();
    unsigned cnt = 0u;
    for (int w = 0; w < NW; ++w) cnt += wcnt[w];
    __syncthreads();
    const unsigned k_eff = cnt < (unsigned)a.top_n ? cnt : (unsigned)a.top_n;
    if (tid == 0) { a.cand_cnt[list] = (int)k_eff; a.cand_tot[list] = (int)cnt; }
    if (k_eff == 0u) return;
    const int idx0 = rec0 * C;
    auto key_of = [&](int i) { return det_key_ord(keys[i], idx0 + i); };
    unsigned long long T = 1ull;
    if (cnt > k_eff)
        T = radix_select64([&](auto f) { for (int i = tid; i < nk; i += YOLO_NT) if (keys[i] != 0u) f(key_of(i)); }, k_eff, hist, sel);

    // ordered compaction: wave w owns the contiguous key slots [w * SEG, (w + 1) * SEG)
    constexpr int SEG = YOLO_SLICE / NW;
    const int s0 = wave * SEG;
    unsigned c = 0u;
    for (int i = s0 + lane; i < s0 + SEG; i += 64) c += __popcll(__ballot(i < nk && keys[i] != 0u && key_of(i) >= T));
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    unsigned run = 0u;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long* out = a.cand + list * a.top_n;
    for (int i = s0 + lane; i < s0 + SEG; i += 64) {
        const bool in = i < nk && keys[i] != 0u;
        const unsigned long long k = in ? key_of(i) : 0ull;
        const bool s = in && k >= T;
        const unsigned long long bm = __ballot(s);
        if (s) {
            const unsigned pos = run + (unsigned)__popcll(bm & lt);
            if (pos < k_eff) out[pos] = k;
        }
        run += (unsigned)__popcll(bm);
    }
}

// launch 2: grid = nl * N (block = level * N + image), YOLO_MT threads: half a block of launch 1, so that the decode's four transcendental chains have 256
// registers per lane instead of 128 and stay clear of scratch; a thread decodes the selected tid and tid + YOLO_MT
__global__ __launch_bounds__(YOLO_MT) void yolo_merge_kernel(const YoloSelect a) {
    __shared__ unsigned long long sbuf[YOLO_KCAP];
    __shared__ unsigned hist[DET_RADIX_BINS];
    __shared__ unsigned sel[2];
    __shared__ unsigned wcnt[YOLO_MT / 64], wtot[YOLO_MT / 64];
    __shared__ unsigned scount;
    constexpr int NW = YOLO_MT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = (int)blockIdx.x / a.N, img = (int)blockIdx.x - l * a.N;
    const YoloLevel& L = a.lv[l];
    const int64_t list0 = L.cand0 + (int64_t)img * L.slices;
    const int* lcnt = a.cand_cnt + list0;
    const int* ltot = a.cand_tot + list0;
    const unsigned long long* cand = a.cand + list0 * a.top_n;

    unsigned mine = 0u, before = 0u;
    for (int s = tid; s < L.slices; s += YOLO_MT) { mine += (unsigned)lcnt[s]; before += (unsigned)ltot[s]; }
    mine = wave_sum(mine);
    before = wave_sum(before);
    if (lane == 0) { wcnt[wave] = mine; wtot[wave] = before; }
    if (tid == 0) scount = 0u;
    for (int i = tid; i < YOLO_KCAP; i += YOLO_MT) sbuf[i] = 0ull;
    __syncthreads();
    unsigned total = 0u, pre_cut = 0u;
    for (int w = 0; w < NW; ++w) { total += wcnt[w]; pre_cut += wtot[w]; }
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
            if (pos < (unsigned)YOLO_KCAP) sbuf[pos] = key;
        }
    });
    __syncthreads();
    bitonic_sort<true>(sbuf, (unsigned)next_pow2((int)k_eff), YOLO_MT);   // the slots past k_eff hold 0, the smallest key: a trained model's handful of winners sorts in a few steps
    const int64_t orow = (int64_t)img * a.nl + l;
    const int64_t obase = orow * a.top_n;   // [N][nl * top_n]: level l's list starts at l * top_n

    // decode of the selected, in selection order; every operation its own rounded fp32 operation
    unsigned done = 0u;   // boxes the earlier halves kept
    for (int h = 0; h * YOLO_MT < (int)k_eff; ++h) {   // uniform
        const int j = tid + h * YOLO_MT;
        const bool real = (unsigned)j < k_eff;
        const unsigned long long kx = sbuf[j];
        const float score = real ? det_key_score(kx) : -1.0f;
        const int idx = real ? det_key_index(kx) : 0;
        float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
        bool ok = false;
        if (real) {
            const int rec = idx / a.C;
            const int cell = rec / a.A, an = rec - cell * a.A;
            const int gy = cell / L.W, gx = cell - gy * L.W;
            const float* t = L.head + ((int64_t)img * L.nrec + rec) * (a.C + 5);
            const float bx = (dm_sigmoid(t[0]) + (float)gx) * L.stride, by = (dm_sigmoid(t[1]) + (float)gy) * L.stride;
            const float bw = dm_exp(t[2]) * L.aw[an], bh = dm_exp(t[3]) * L.ah[an];   // dm_exp saturates: +inf is possible and clips to the canvas
            const float hw = bw * 0.5f, hh = bh * 0.5f;
            box.x = clampf(bx - hw, a.canvas_w); box.y = clampf(by - hh, a.canvas_h);   // clampf keeps a NaN
            box.z = clampf(bx + hw, a.canvas_w); box.w = clampf(by + hh, a.canvas_h);
            const bool nan = box.x != box.x || box.y != box.y || box.z != box.z || box.w != box.w;
            ok = !nan && (box.z - box.x >= a.min_wh) && (box.w - box.y >= a.min_wh);
        }
        const unsigned long long bm = __ballot(ok);
        __syncthreads();   // the previous half's reads of wcnt
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(bm);
        __syncthreads();
        unsigned run = 0u, tot = 0u;
        for (int w = 0; w < NW; ++w) { if (w < wave) run += wcnt[w]; tot += wcnt[w]; }
        if (ok) {
            const int64_t o = obase + done + run + (unsigned)__popcll(bm & ((1ull << lane) - 1ull));
            *(float4*)(a.out_boxes + o * 4) = box;
            a.out_scores[o] = score;
            a.out_labels[o] = idx % a.C + 1;
        }
        done += tot;
    }
    for (int j = (int)done + tid; j < a.top_n; j += YOLO_MT) {
        const int64_t o = obase + j;
        *(float4*)(a.out_boxes + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        a.out_scores[o] = -1.0f;
        a.out_labels[o] = 0;
    }
    if (tid == 0) { a.out_cnt[orow] = (int)done; a.out_total[orow] = (int)pre_cut; }
}

// one float4 of the output per thread; Cc4 / Ct4: channels of the coarse map / of the output, in float4s
__global__ __launch_bounds__(256) void concat_up2x_kernel(const float4* __restrict__ coarse, const float4* __restrict__ skip, float4* __restrict__ out,
                                                          int64_t total, int Hc, int Wc, int Cc4, int Ct4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t pix = i / Ct4;
    const int c = (int)(i - pix * Ct4);
    if (c >= Cc4) {
        out[i] = skip[pix * (Ct4 - Cc4) + (c - Cc4)];
        return;
    }
    const int W = 2 * Wc, H = 2 * Hc;
    const int x = (int)(pix % W);
    const int64_t ny = pix / W;
    const int y = (int)(ny % H);
    const int64_t n = ny / H;
    out[i] = coarse[((n * Hc + (y >> 1)) * Wc + (x >> 1)) * Cc4 + c];
}

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int yolo_lists(int nl, int N, const int* grid_hw, int A, int C, int top_n, int64_t* lists) {
    if (nl < 1 || nl > ISEGMI_YOLO_MAX_LEVELS || N < 1 || A < 1 || A > YOLO_MAX_A || C < 1 || C > 256 || top_n < 1 || top_n > YOLO_KCAP) return -1;
    const int rs = yolo_slice_records(C);
    int64_t n = 0;
    for (int l = 0; l < nl; ++l) {
        const int64_t H = grid_hw[2 * l], W = grid_hw[2 * l + 1];
        if (H < 1 || W < 1 || H > 32768 || W > 32768 || H * W * A * C > 0x7fffffff) return -1;
        n += (int64_t)N * ((H * W * A + rs - 1) / rs);
    }
    if (n > 0x7fffffff) return -1;
    *lists = n;
    return 0;
}

}  // namespace

int yolo_slice_records(int C) { return C >= 1 && C <= 256 ? YOLO_SLICE / (C + 5) : -1; }

int64_t yolo_select_workspace_bytes(int nl, int N, const int* grid_hw, int A, int C, int top_n) {
    int64_t lists = 0;
    if (grid_hw == nullptr || yolo_lists(nl, N, grid_hw, A, C, top_n, &lists)) return -1;
    return align256(lists * top_n * 8) + 2 * align256(lists * 4);
}

int yolo_select_launch(int nl, int N, const float* const* d_heads, const int* grid_hw, const int* strides, const float* anchors_wh, int A, int C, int top_n,
                       float conf_thresh, int multi_label, float min_wh, int canvas_w, int canvas_h, void* d_ws, int64_t ws_bytes, float* d_out_boxes,
                       float* d_out_scores, int* d_out_labels, int* d_out_cnt, int* d_out_total, hipStream_t st) {
    ARG_CHECK(d_heads && grid_hw && strides && anchors_wh, "yolo_select: null host array");
    ARG_CHECK(nl >= 1 && nl <= ISEGMI_YOLO_MAX_LEVELS, "yolo_select: 1-3 levels");
    ARG_CHECK(N >= 1 && A >= 1 && A <= YOLO_MAX_A && C >= 1 && C <= 256, "yolo_select sizes: N >= 1, A 1..8, C 1..256");
    ARG_CHECK(top_n >= 1 && top_n <= YOLO_KCAP, "yolo_select: top_n must be 1..1024");
    ARG_CHECK(conf_thresh >= 0.0f && min_wh >= 0.0f, "yolo_select: conf_thresh and min_wh are non-negative numbers");
    ARG_CHECK(multi_label == 0 || multi_label == 1, "yolo_select: multi_label is 0 or 1");
    ARG_CHECK(canvas_w >= 1 && canvas_h >= 1, "yolo_select: canvas");
    ARG_CHECK(d_ws && d_out_boxes && d_out_scores && d_out_labels && d_out_cnt && d_out_total, "yolo_select: null device pointer");
    int64_t lists = 0;
    ARG_CHECK(yolo_lists(nl, N, grid_hw, A, C, top_n, &lists) == 0, "yolo_select: a grid is empty or a level holds over 2^31 (anchor, class) pairs");
    ARG_CHECK(ws_bytes >= yolo_select_workspace_bytes(nl, N, grid_hw, A, C, top_n), "yolo_select: workspace too small (isegmi_op_yolo_select_workspace)");
    YoloSelect a;
    memset(&a, 0, sizeof(a));
    a.nl = nl; a.N = N; a.A = A; a.C = C; a.top_n = top_n; a.rs = yolo_slice_records(C); a.multi_label = multi_label;
    a.thr = conf_thresh; a.min_wh = min_wh; a.canvas_w = (float)canvas_w; a.canvas_h = (float)canvas_h;
    int blk = 0;
    int64_t off = 0;
    for (int l = 0; l < nl; ++l) {
        ARG_CHECK(d_heads[l] != nullptr, "yolo_select: null level pointer");
        ARG_CHECK(strides[l] >= 1, "yolo_select: stride");
        YoloLevel& L = a.lv[l];
        L.head = d_heads[l]; L.H = grid_hw[2 * l]; L.W = grid_hw[2 * l + 1]; L.nrec = L.H * L.W * A;
        L.slices = (L.nrec + a.rs - 1) / a.rs;
        L.blk0 = blk; L.cand0 = off;
        L.stride = (float)strides[l];
        for (int k = 0; k < A; ++k) { L.aw[k] = anchors_wh[(l * A + k) * 2]; L.ah[k] = anchors_wh[(l * A + k) * 2 + 1]; }
        blk += N * L.slices;
        off += (int64_t)N * L.slices;
    }
    a.cand = (unsigned long long*)d_ws;
    a.cand_cnt = (int*)((char*)d_ws + align256(lists * top_n * 8));
    a.cand_tot = (int*)((char*)a.cand_cnt + align256(lists * 4));
    a.out_boxes = d_out_boxes; a.out_scores = d_out_scores; a.out_labels = d_out_labels; a.out_cnt = d_out_cnt; a.out_total = d_out_total;
    hipLaunchKernelGGL(yolo_slice_kernel, dim3(blk), dim3(YOLO_NT), 0, st, a);
    hipLaunchKernelGGL(yolo_merge_kernel, dim3(nl * N), dim3(YOLO_MT), 0, st, a);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int concat_up2x_launch(const float* coarse, int N, int Hc, int Wc, int Cc, const float* skip, int Cs, float* out, hipStream_t st) {
    ARG_CHECK(coarse && skip && out, "concat_up2x: null pointer");
    ARG_CHECK(N >= 1 && Hc >= 1 && Wc >= 1 && Hc <= 16384 && Wc <= 16384, "concat_up2x sizes");
    ARG_CHECK(Cc >= 32 && Cs >= 32 && Cc % 32 == 0 && Cs % 32 == 0, "concat_up2x: Cc and Cs are positive multiples of 32");
    const int Ct4 = (Cc + Cs) / 4;
    const int64_t total = (int64_t)N * (2 * Hc) * (2 * Wc) * Ct4;
    ARG_CHECK(total <= (int64_t)0x7fffffff * 256, "concat_up2x: output too large for one launch");
    hipLaunchKernelGGL(concat_up2x_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float4*)coarse, (const float4*)skip, (float4*)out,
                       total, Hc, Wc, Cc / 4, Ct4);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_yolo_slice_records(int C) { return yolo_slice_records(C); }
extern "C" int64_t isegmi_op_yolo_select_workspace(int nl, int N, const int32_t* grid_hw, int A, int C, int top_n) {
    return yolo_select_workspace_bytes(nl, N, grid_hw, A, C, top_n);
}
extern "C" int isegmi_op_yolo_select(int nl, int N, const float* const* d_heads, const int32_t* grid_hw, const int32_t* strides, const float* anchors_wh, int A,
                                     int C, int top_n, float conf_thresh, int multi_label, float min_wh, int canvas_w, int canvas_h, void* d_ws,
                                     int64_t ws_bytes, float* d_out_boxes, float* d_out_scores, int32_t* d_out_labels, int32_t* d_out_cnt,
                                     int32_t* d_out_total, void* stream) {
    return yolo_select_launch(nl, N, d_heads, grid_hw, strides, anchors_wh, A, C, top_n, conf_thresh, multi_label, min_wh, canvas_w, canvas_h, d_ws, ws_bytes,
                              d_out_boxes, d_out_scores, d_out_labels, d_out_cnt, d_out_total, (hipStream_t)stream);
}
extern "C" int isegmi_op_concat_up2x(const float* d_coarse, int N, int Hc, int Wc, int Cc, const float* d_skip, int Cs, float* d_out, void* stream) {
    return concat_up2x_launch(d_coarse, N, Hc, Wc, Cc, d_skip, Cs, d_out, (hipStream_t)stream);
}
