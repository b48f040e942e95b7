// pose_handoff.hip -- Keypoint R-CNN detections -> Pose2Seg's packed person keypoints, on the device.
//
// One workgroup per image.  Of image n's detection slots j < count[n] the candidates are those with score > person_thresh; the min(#candidates, K) best
// are kept, ordered by score descending, equal scores by slot ascending.  The rank of a candidate is COUNTED (candidates that beat it), so the input need
// not be sorted and the result does not depend on the order in which anything runs; image n's rows start at the sum of the kept counts of the images
// before it, which the workgroup recomputes itself (no atomics, no second launch).  O(N cap / 256) barriers and O(cap^2 / 256) compares per thread.
#include "common.h"
#include "../../include/isegmi.h"

namespace isegmi {

constexpr int kHandoffThreads = 256;
constexpr int kHandoffNK = 17;
constexpr int kHandoffMaxCap = 4096;   // 2 x 16 KiB of LDS

// detections of image m that pass the person threshold (every thread gets the sum; all threads must call)
__device__ __forceinline__ int handoff_candidates(const float* __restrict__ score, int live, float person_thresh) {
    int c = 0;
    for (int j0 = 0; j0 < live; j0 += kHandoffThreads) {
        const int j = j0 + (int)threadIdx.x;
        c += __syncthreads_count(j < live && score[j] > person_thresh);
    }
    return c;
}

__global__ __launch_bounds__(kHandoffThreads) void pose_handoff_kernel(const float* __restrict__ score, const int32_t* __restrict__ count,
                                                                       const float* __restrict__ kpt, const float* __restrict__ kscore,
                                                                       const float* __restrict__ ratios, int cap, float person_thresh, float kp_thresh, int K,
                                                                       float* __restrict__ kpts_out, float* __restrict__ score_out,
                                                                       int32_t* __restrict__ src_slot, int32_t* __restrict__ count_out) {
    extern __shared__ __align__(16) unsigned char handoff_lds[];
    float* s_score = (float*)handoff_lds;            // [cap] scores of the live slots
    int32_t* s_sel = (int32_t*)(s_score + cap);      // [cap] rank -> slot of the kept persons
    const int n = blockIdx.x, tid = threadIdx.x;
    // first output row: the kept counts of the images in front of this one
    int row0 = 0;
    for (int m = 0; m < n; ++m) {
        const int live = min(max(count[m], 0), cap);
        row0 += min(handoff_candidates(score + (int64_t)m * cap, live, person_thresh), K);
    }
    const int live = min(max(count[n], 0), cap);
    const float* sc = score + (int64_t)n * cap;
    const int kept = min(handoff_candidates(sc, live, person_thresh), K);
    for (int j = tid; j < live; j += kHandoffThreads) s_score[j] = sc[j];
    __syncthreads();
    // rank by counting: candidates with a larger score, or the same score in a lower slot
    for (int j = tid; j < live; j += kHandoffThreads) {
        const float s = s_score[j];
        if (!(s > person_thresh)) continue;
        int rank = 0;
        for (int i = 0; i < live; ++i) {
            const float t = s_score[i];
            rank += (t > person_thresh && (t > s || (t == s && i < j))) ? 1 : 0;
        }
        if (rank < kept) s_sel[rank] = j;
    }
    __syncthreads();
    for (int r = tid; r < K; r += kHandoffThreads) {
        const bool on = r < kept;
        score_out[(int64_t)n * K + r] = on ? s_score[s_sel[r]] : 0.0f;
        src_slot[(int64_t)n * K + r] = on ? s_sel[r] : -1;
    }
    if (tid == 0) count_out[n] = kept;
    const float rw = ratios[2 * n], rh = ratios[2 * n + 1];
    const int per = kHandoffNK * 3;
    for (int i = tid; i < kept * per; i += kHandoffThreads) {
        const int r = i / per, e = i - r * per, k = e / 3, c = e - k * 3;
        const int64_t det = (int64_t)n * cap + s_sel[r];
        float v;
        if (c == 2) v = kscore[det * kHandoffNK + k] > kp_thresh ? 2.0f : 0.0f;
        else v = kpt[(det * kHandoffNK + k) * 3 + c] * (c == 0 ? rw : rh);   // one fp32 multiplication, as pack_keypoint_records_kernel
        kpts_out[((int64_t)row0 + r) * per + e] = v;
    }
}

// det.score of a Pose2Seg step fed by the hand-off: the live slots take the persons' box scores, the others stay as the mask kernel left them
__global__ void pose_scores_kernel(const float* __restrict__ in, const int32_t* __restrict__ counts, int N, int K, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    if (i % K < counts[i / K]) out[i] = in[i];
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_pose_handoff(const float* d_score, const int32_t* d_count, const float* d_kpt, const float* d_kscore, const float* d_ratios_wh, int N,
                                      int cap, int NK, float person_thresh, float kp_thresh, int K, float* d_kpts_out, float* d_score_out,
                                      int32_t* d_src_slot, int32_t* d_count_out, void* stream) {
    ARG_CHECK(NK == kHandoffNK, "num_keypoints: Pose2Seg takes COCO's 17 keypoints");
    ARG_CHECK(N >= 1 && N <= 65535, "batch size");
    ARG_CHECK(cap >= 1 && cap <= kHandoffMaxCap, "cap: 1..4096 detection slots per image");
    ARG_CHECK(K >= 1 && (int64_t)N * K <= 65535, "K: max_instances >= 1, N * K <= 65535");
    ARG_CHECK(d_score && d_count && d_kpt && d_kscore && d_ratios_wh && d_kpts_out && d_score_out && d_src_slot && d_count_out, "null device pointer");
    hipLaunchKernelGGL(pose_handoff_kernel, dim3(N), dim3(kHandoffThreads), (size_t)cap * 8, (hipStream_t)stream, d_score, d_count, d_kpt, d_kscore, d_ratios_wh,
                       cap, person_thresh, kp_thresh, K, d_kpts_out, d_score_out, d_src_slot, d_count_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

extern "C" int isegmi_op_pose_scores(const float* d_scores_in, const int32_t* d_counts, int N, int K, float* d_scores_out, void* stream) {
    ARG_CHECK(N >= 1 && K >= 1 && (int64_t)N * K <= 65535, "sizes");
    ARG_CHECK(d_scores_in && d_counts && d_scores_out, "null device pointer");
    hipLaunchKernelGGL(pose_scores_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, (hipStream_t)stream, d_scores_in, d_counts, N, K, d_scores_out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}
