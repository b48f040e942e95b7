// detsoftmax.h -- the box head's class softmax of one row by one wave, in one place: shared by softmax_rows_kernel (csrc/rcnn_ops.hip, the plain tail's
// probability tensor) and the test-time-augmentation candidate stage (csrc/bbox_aug.hip), which thresholds the same probabilities without storing them.
// The exponentials and the divisions run across the lanes; the max is order-free; the SUM keeps the oracle's sequential order
// (s = ((e0 + e1) + e2) + ...), every lane adding the row's exponentials from LDS in class order.
#pragma once
#include "detmath.h"

namespace isegmi {

constexpr int SOFTMAX_MAXC = 320;
constexpr int SOFTMAX_Q = SOFTMAX_MAXC / 64;   // classes per lane: lane owns c = lane + 64 q

// the two roundings every probability goes through: p = softmax_prob(softmax_exp(x, m), sum)
__device__ __forceinline__ float softmax_exp(float x, float m) { return dm_exp(x - m); }
__device__ __forceinline__ float softmax_prob(float e, float sum) { return dm_div(e, sum); }

// Row `a` of C <= SOFTMAX_MAXC logits.  All 64 lanes of one wave call; `ex` is that wave's own LDS row of SOFTMAX_MAXC floats (reusable right after the
// call returns: every lane has read it, behind the second wave barrier -- a scheduling fence, no arithmetic).  *m = the row's max, v[q] = dm_exp(a[lane + 64 q] - m) for the lane's classes below C, returns the sum.
__device__ __forceinline__ float softmax_row_wave(const float* __restrict__ a, int C, int lane, float* ex, float (&v)[SOFTMAX_Q], float* m_out) {
    float m = -3.0e38f;
#pragma unroll
    for (int q = 0; q < SOFTMAX_Q; ++q) {
        const int c = lane + 64 * q;
        v[q] = c < C ? a[c] : -3.0e38f;
        m = v[q] > m ? v[q] : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const float t = __shfl_xor(m, off, 64); m = t > m ? t : m; }
#pragma unroll
    for (int q = 0; q < SOFTMAX_Q; ++q) {
        const int c = lane + 64 * q;
        if (c < C) { v[q] = softmax_exp(v[q], m); ex[c] = v[q]; }
    }
    __builtin_amdgcn_wave_barrier();
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum = sum + ex[c];
    __builtin_amdgcn_wave_barrier();
    *m_out = m;
    return sum;
}

}  // namespace isegmi
