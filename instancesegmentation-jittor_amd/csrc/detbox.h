// detbox.h -- the device code that makes the detectors' discrete decisions, in one place: ordered sort keys, box decode / clip / min-size, the exact IoU
// predicate, the block-wide bitonic sort, the radix select, the 64 x 64 suppression-matrix tile and the chunk resolve of the greedy scan.  Shared by csrc/select.hip
// (top-k), csrc/rcnn_ops.hip (RPN, box head), csrc/retinanet_ops.hip and csrc/yolo_ops.hip; every result here is pinned bit for bit against oracle/ora_ops.c by the tests of those files.
// Box arithmetic follows the oracle operation for operation (compile with -ffp-contract=off, see detmath.h).
#pragma once
#include "../../include/isegmi.h"
#include "detmath.h"

namespace isegmi {

// ------------------------------------------------------------------ ordered keys
// KEY ORDER CONTRACT.  Keys compare as floats, not as bit patterns: -0.0 and +0.0 are EQUAL (the lower
// index wins, as in ora_topk, ora_nms's comparator, torch.topk and sort), -inf < every finite key < +inf,
// subnormals keep their value.  f2ord() maps both zeros to one sort key; a returned value is rebuilt from
// that key, so a selected -0.0 comes back as +0.0 (every other value comes back bit for bit).  NaN keys are
// outside the contract: a comparator-based reference has no total order with them.
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) return 0x80000000u;  // -0.0 == +0.0: one key for both, the index decides
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
    const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(u);
}
// 64-bit key whose unsigned DESCENDING order is (score descending, index ascending): ordered score << 32 | ~index
__device__ __forceinline__ unsigned long long det_key_ord(unsigned ord, int idx) {
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
}
__device__ __forceinline__ unsigned long long det_key(float score, int idx) { return det_key_ord(f2ord(score), idx); }
__device__ __forceinline__ float det_key_score(unsigned long long key) { return ord2f((unsigned)(key >> 32)); }
__device__ __forceinline__ int det_key_index(unsigned long long key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

// ------------------------------------------------------------------ box coder
// BoxCoder.decode with the legacy +1 widths and the log(1000/16) clamp (the oracle's decode_box)
__device__ __forceinline__ float4 decode_box(const float4 a, const float4 d, float wx, float wy, float ww, float wh) {
    const float clipv = 4.135166556742356f;
    const float widths = a.z - a.x + 1.0f, heights = a.w - a.y + 1.0f;
    const float ctr_x = a.x + 0.5f * widths, ctr_y = a.y + 0.5f * heights;
    const float dx = dm_div(d.x, wx), dy = dm_div(d.y, wy);
    float dw = dm_div(d.z, ww), dh = dm_div(d.w, wh);
    dw = dw < clipv ? dw : clipv;
    dh = dh < clipv ? dh : clipv;
    const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
    const float pw = dm_exp(dw) * widths, ph = dm_exp(dh) * heights;
    float4 o;
    o.x = pcx - 0.5f * pw;
    o.y = pcy - 0.5f * ph;
    o.z = pcx + 0.5f * pw - 1.0f;
    o.w = pcy + 0.5f * ph - 1.0f;
    return o;
}
__device__ __forceinline__ float clampf(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }
__device__ __forceinline__ float4 clip_box(float4 b, float im_w, float im_h) {
    const float mx = im_w - 1.0f, my = im_h - 1.0f;
    b.x = clampf(b.x, mx); b.y = clampf(b.y, my); b.z = clampf(b.z, mx); b.w = clampf(b.w, my);
    return b;
}
// remove_small_boxes on the legacy +1 sides
__device__ __forceinline__ bool box_min_size_ok(const float4 b, float min_size) {
    const float ws = b.z - b.x + 1.0f, hs = b.w - b.y + 1.0f;
    return ws >= min_size && hs >= min_size;
}
__device__ __forceinline__ float iou_one(const float4 a, const float4 b, float one) {
    const float aa = (a.z - a.x + one) * (a.w - a.y + one);
    const float ab = (b.z - b.x + one) * (b.w - b.y + one);
    const float xx1 = a.x > b.x ? a.x : b.x, yy1 = a.y > b.y ? a.y : b.y;
    const float xx2 = a.z < b.z ? a.z : b.z, yy2 = a.w < b.w ? a.w : b.w;
    float w = xx2 - xx1 + one, h = yy2 - yy1 + one;
    w = w > 0.0f ? w : 0.0f;
    h = h > 0.0f ? h : 0.0f;
    const float inter = w * h;
    return dm_div(inter, aa + ab - inter);
}

// Division-free, EXACT form of `RN(inter / uni) > thr` (ge: `>= thr`).  RN is monotone, so the fp32 quotient
// exceeds thr iff the real quotient lies beyond the midpoint between thr and its fp32 neighbour (ties go to the
// even mantissa).  inter, uni are 24-bit, the midpoint 25-bit: their product is exact in fp64.  ~6 instructions
// instead of an IEEE-correct fp32 division (~40) in the innermost NMS loop; bit-identical to the oracle's division.
struct IouThr {
    double m;       // midpoint
    bool tie_true;  // result when inter == m * uni exactly
};
__device__ __forceinline__ IouThr make_iou_thr(float thr, int ge) {
    IouThr t;
    const unsigned b = __float_as_uint(thr);  // thr > 0
    if (ge) {  // q >= thr  <=>  x >= mid(pred(thr), thr) (tie -> thr iff thr's mantissa is even)
        const float lo = __uint_as_float(b - 1u);
        t.m = 0.5 * ((double)lo + (double)thr);
        t.tie_true = (b & 1u) == 0u;
    } else {   // q > thr   <=>  x >= mid(thr, succ(thr)) (tie -> succ iff succ's mantissa is even)
        const float hi = __uint_as_float(b + 1u);
        t.m = 0.5 * ((double)thr + (double)hi);
        t.tie_true = ((b + 1u) & 1u) == 0u;
    }
    return t;
}
__device__ __forceinline__ bool iou_exceeds(const float4 a, const float4 b, float one, const IouThr t) {
    const float aa = (a.z - a.x + one) * (a.w - a.y + one);
    const float ab = (b.z - b.x + one) * (b.w - b.y + one);
    const float xx1 = a.x > b.x ? a.x : b.x, yy1 = a.y > b.y ? a.y : b.y;
    const float xx2 = a.z < b.z ? a.z : b.z, yy2 = a.w < b.w ? a.w : b.w;
    float w = xx2 - xx1 + one, h = yy2 - yy1 + one;
    w = w > 0.0f ? w : 0.0f;
    h = h > 0.0f ? h : 0.0f;
    const float inter = w * h;
    const float uni = aa + ab - inter;
    if (!(uni > 0.0f)) return false;  // 0/0 or negative union: NaN / non-positive quotient never exceeds thr > 0
    const double lhs = (double)inter, rhs = t.m * (double)uni;
    return lhs > rhs || (lhs == rhs && t.tie_true);
}

// The `ge` / `nms_flags` argument of the engine-level launches is the OR of the App. A.6 forks (include/isegmi.h): ISEGMI_NMS_GE (1) suppress on
// iou >= thr instead of >; ISEGMI_NMS_NO_PLUS_ONE (2) plain areas instead of the legacy +1; ISEGMI_NMS_INDEX_ORDER (4, box post-processing only) a class's
// kept detections in ascending proposal index (the CPU NMS's nonzero order) instead of score order.
__device__ __forceinline__ float nms_one(int flags) { return (flags & ISEGMI_NMS_NO_PLUS_ONE) ? 0.0f : 1.0f; }

// ------------------------------------------------------------------ bitonic sort
__host__ __device__ __forceinline__ int next_pow2(int n) { int p = 2; while (p < n) p <<= 1; return p; }
// Block-wide bitonic sort of P (a power of two >= 2) 64-bit keys in LDS, descending or ascending; nt = threads of the block (all of them call).  P and nt
// fold where the caller passes constants.  The index arithmetic is unsigned: t / stride and t % stride are then one division, not two signed ones (a signed
// form cost retina_sort_kernel 29 %).  Ends on a barrier.
template <bool DESC>
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, const unsigned P, const unsigned nt) {
    for (unsigned size = 2; size <= P; size <<= 1)
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned t = threadIdx.x; t < P / 2; t += nt) {
                const unsigned lo = ((t / stride) * stride * 2) + (t % stride), hi = lo + stride;
                const bool fwd = ((lo & size) == 0);  // this merge runs in the sort's own direction
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((fwd == DESC) ? (x < y) : (x > y)) { keys[lo] = y; keys[hi] = x; }
            }
            __syncthreads();
        }
}

// ------------------------------------------------------------------ radix select
constexpr int DET_RADIX_BINS = 2048;   // 11-bit digits: 6 passes over a 64-bit key
// The k-th largest of `total` >= k unique 64-bit keys (k >= 1): six 11-bit digits from the top, one LDS histogram each.  each(f) calls f(key) for every key,
// block-wide, in any order.  All threads return the same value.
template <class Each>
__device__ unsigned long long radix_select64(Each each, unsigned k, unsigned* hist, unsigned* sel) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long prefix = 0ull;
    unsigned kk = k;
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = 55 - 11 * pass;
        for (int i = tid; i < DET_RADIX_BINS; i += blockDim.x) hist[i] = 0u;
        __syncthreads();
        each([&](unsigned long long key) {
            const bool match = pass == 0 || (key >> (shift + 11)) == (prefix >> (shift + 11));
            if (match) atomicAdd(&hist[(unsigned)(key >> shift) & (DET_RADIX_BINS - 1)], 1u);   // a count: order-free
        });
        __syncthreads();
        if (tid < 64) {   // wave 0: lane owns 32 consecutive bins; suffix sums across lanes, then a walk down its own bins
            constexpr int PER = DET_RADIX_BINS / 64;
            unsigned tsum = 0u;
            for (int j = 0; j < PER; ++j) tsum += hist[lane * PER + j];
            unsigned v = tsum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_down(v, off, 64);
                if (lane + off < 64) v += o;
            }
            unsigned above = v - tsum;
            for (int j = PER - 1; j >= 0; --j) {
                const unsigned h = hist[lane * PER + j];
                if (above < kk && above + h >= kk) { sel[0] = (unsigned)(lane * PER + j); sel[1] = kk - above; }
                above += h;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)sel[0] << shift;
        kk = sel[1];
        __syncthreads();
    }
    return prefix;
}

// ------------------------------------------------------------------ suppression-matrix tile
// The suppression matrix of n boxes in visiting order: bit b of word w of row i set iff box j = 64w + b comes after box i, is eligible and
// IoU(i, j) exceeds the threshold.  Only words on and right of the diagonal exist; wave-task `pair` owns rows 64r..64r+63 (lane = row) x word w, r <= w.
__device__ __forceinline__ void tri_pair(int pair, int& r, int& w) {
    w = 0;
    while ((w + 1) * (w + 2) / 2 <= pair) ++w;
    r = pair - w * (w + 1) / 2;
}
// this wave's 64 column boxes into its own LDS row; no block-level barrier
__device__ __forceinline__ void nms_stage_cols(float4* cols, int lane, const float4 box) {
    cols[lane] = box;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's own LDS writes have landed
}
// row i's word w from the 64 column boxes cols[0..64) (broadcast reads); eligible(j, b) says whether column j = 64w + b may be suppressed at all
template <class Eligible>
__device__ __forceinline__ unsigned long long nms_tile_word(const float4 mine, const float4* cols, int i, int w, float one, const IouThr T, Eligible eligible) {
    unsigned long long m = 0ull;
#pragma unroll 8
    for (int b = 0; b < 64; ++b) {
        const int j = (w << 6) + b;
        const bool sup = j > i && eligible(j, b) && iou_exceeds(mine, cols[b], one, T);
        m |= sup ? (1ull << b) : 0ull;
    }
    return m;
}

// ------------------------------------------------------------------ chunk resolve
// Greedy NMS inside one chunk of 64 from its diagonal words alone (lane b holds d = box b's word: its later chunk-mates that it suppresses): a 64-step
// scalar chain (readlane / bitcmp / andn2: no IoU, no memory).  alive (uniform): the chunk's candidates; returns the survivors = the kept boxes.
__device__ __forceinline__ unsigned long long nms_resolve_chunk(unsigned long long alive, const unsigned long long d) {
    const int dlo = (int)(unsigned)d, dhi = (int)(unsigned)(d >> 32);
#pragma unroll
    for (int b = 0; b < 64; ++b) {  // box b survives => it strikes its later chunk-mates
        const unsigned long long db = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, b) << 32) |
                                      (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, b);
        alive &= ((alive >> b) & 1ull) ? ~db : ~0ull;
    }
    return alive;
}

}  // namespace isegmi
