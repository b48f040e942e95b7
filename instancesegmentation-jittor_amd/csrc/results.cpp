// results.cpp -- device-side COCO output of a step: run-length encoding of the masks the last postprocess /
// paste produced, ONE fixed-size record block per batch (the unit the N = 1 path downloads and the N > 1 path all-gathers over RCCL), and
// its asynchronous download.  Stands where upstream turns predictions into COCO json: maskrcnn-benchmark inference() ->
// prepare_for_coco_segmentation (README.md:344-347), Yolact eval.py Detections.add_bbox / add_mask -> dump (README.md:243-249).
//
// Record block of a batch of N images, K = detection capacity per image (byte offsets are multiples of 8):
//   [status  i32 x 4]            total runs, total characters, overflow bits (1 runs, 2 characters: raise the "rle_cap_*" params), 0
//   [box     N*K*4]              Mask R-CNN, Pose2Seg: f32 xyxy in ORIGINAL image coordinates (det.box_resized); Yolact: i64 xyxy (det.box_int)
//   [count   i32 x N]
//   [score   f32 x N*K]
//   [label   i32 x N*K]          Mask R-CNN: 1..80; Yolact: class 0..79; Pose2Seg: 1
//   [mscore  f32 x N*K]          YOLACT++ only (mask re-scoring)
//   [str_off i32 x (N*K + 1)]    characters of slot (n, k): chars[str_off[n*K+k] .. str_off[n*K+k+1])
//   [pad to 8]
//   [chars   u8 x cap_chars]     pycocotools "counts" strings, back to back
//
// Box-only block (Faster R-CNN: a Mask R-CNN-family engine with "mask_on" 0), every section starting on a multiple of 8 bytes:
//   [status  i32 x 4 = 0][box f32 x N*K*4, original-image xyxy][count i32 x N][score f32 x N*K][label i32 x N*K]      no str_off, no characters
//
// Keypoint block (Keypoint R-CNN: "keypoint_on" 1): the box-only block with two more sections behind label, each on a multiple of 8 bytes:
//   ... [label i32 x N*K][kpt f32 x N*K*NK*3, (x, y) in original-image coordinates, v][kscore f32 x N*K*NK]           NK keypoints per detection
#include <string.h>

#include "engine.h"

namespace isegmi {
int rle_encode_launch(const isegmi_rle_args* a, hipStream_t st);

// Pose2Seg (kind 3) takes the Mask R-CNN record form (f32 boxes, i32 labels) with K = its max_instances
static int det_cap(Engine& e) {
    return e.kind == 1 ? (int)e.param("max_num_detections", 100) : e.kind == 3 ? pose2seg_det_cap(e) : maskrcnn_det_cap(e);
}
// Default RLE capacities per image: a blob mask costs ~2 runs per column it spans and ~1.7 characters per run, so K masks as wide as the
// network canvas need ~4 K W runs; the fixed 256 Ki of round 3 was marginal at 640 px and short at 1500 px with K = 100.  An
// overflow is not fatal any more (isegmi.pipeline.run_record_loop raises these parameters and redoes the step), this only makes it rare.
static int64_t rle_cap_default(Engine& e) {
    const int64_t side = e.H > e.W ? e.H : e.W;
    const int64_t c = 4ll * det_cap(e) * side;
    return (c < 262144 ? 262144 : c) * e.max_batch;
}
static int rle_cap_chars(Engine& e) { return (int)e.param("rle_cap_chars", (float)(2 * rle_cap_default(e))); }
static int rle_cap_runs(Engine& e) {
    int c = (int)e.param("rle_cap_runs", (float)rle_cap_default(e));
    return (c + 1023) / 1024 * 1024;
}

struct Section { const char* buf; int64_t bytes; };

static int64_t align8(int64_t v) { return (v + 7) & ~7ll; }

// sections of the record block in order (chars excluded); `with_mscore`: YOLACT++
static int record_layout(Engine& e, int N, std::vector<Section>* out, int64_t* chars_off, int64_t* total) {
    const int K = det_cap(e);
    const bool y = e.kind == 1;
    const bool ms = y && e.convs.count("maskiou_net.2") != 0;
    std::vector<Section> s;
    s.push_back({"rle.status", 16});
    s.push_back({y ? "det.box_int" : "det.box_resized", (int64_t)N * K * (y ? 32 : 16)});
    s.push_back({"det.count", (int64_t)N * 4});
    s.push_back({"det.score", (int64_t)N * K * 4});
    s.push_back({y ? "det.class" : "det.label", (int64_t)N * K * 4});
    if (ms) s.push_back({"det.mask_score", (int64_t)N * K * 4});
    s.push_back({"rle.str_off", ((int64_t)N * K + 1) * 4});
    int64_t off = 0;
    for (auto& x : s) off += x.bytes;
    off = align8(off);
    if (out) *out = s;
    if (chars_off) *chars_off = off;
    if (total) *total = off + rle_cap_chars(e);
    return ISEGMI_OK;
}

static bool box_only(Engine& e) { return e.kind == 2 && !maskrcnn_mask_on(e); }

// byte offsets of the box-only block's sections for n image slots
struct BoxRecordLayout { int64_t box, count, score, label, total; };
static BoxRecordLayout box_record_layout(int n, int K) {
    BoxRecordLayout l;
    l.box = 16;
    l.count = align8(l.box + (int64_t)n * K * 16);
    l.score = align8(l.count + (int64_t)n * 4);
    l.label = align8(l.score + (int64_t)n * K * 4);
    l.total = align8(l.label + (int64_t)n * K * 4);
    return l;
}

// the keypoint block: the box-only sections, then kpt and kscore
struct KeypointRecordLayout { BoxRecordLayout b; int64_t kpt, kscore, total; };
static KeypointRecordLayout keypoint_record_layout(int n, int K, int NK) {
    KeypointRecordLayout l;
    l.b = box_record_layout(n, K);
    l.kpt = l.b.total;
    l.kscore = align8(l.kpt + (int64_t)n * K * NK * 12);
    l.total = align8(l.kscore + (int64_t)n * K * NK * 4);
    return l;
}

// RLE of det.masks (the planes the last yolact_postprocess / maskrcnn_paste wrote) on the results stream.
int eng_rle(Engine& e, const int32_t* h_image_hw) {
    const int N = e.last_N;
    if (box_only(e)) { set_error("rle: the engine is box-only (mask_on 0, MODEL.MASK_ON False): there are no masks to encode"); return ISEGMI_ERR_STATE; }
    if (N <= 0) { set_error("rle before forward"); return ISEGMI_ERR_STATE; }
    auto mit = e.bufs.find("det.masks");
    if (mit == e.bufs.end() || mit->second.shape.size() != 4 || mit->second.shape[0] != N) { set_error("rle: run postprocess / paste of this batch first"); return ISEGMI_ERR_STATE; }
    const int K = (int)mit->second.shape[1], ph = (int)mit->second.shape[2], pw = (int)mit->second.shape[3];
    hipStream_t rs = eng_results_stream(e);
    isegmi_rle_args a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.K = K; a.plane_h = ph; a.plane_w = pw; a.cap_runs = rle_cap_runs(e); a.cap_chars = rle_cap_chars(e);
    a.d_masks = (const uint8_t*)mit->second.d;
    a.d_count = (const int32_t*)e.bufs["det.count"].d;
    {   // the windows the paste / mask assembly kernel wrote next to the planes: only they are read (Pose2Seg writes whole planes and leaves none)
        auto wit = e.bufs.find("det.mask_window");
        if (wit != e.bufs.end() && wit->second.d != nullptr && wit->second.shape.size() == 3 && wit->second.shape[0] == N && wit->second.shape[1] == K)
            a.d_windows = (const int32_t*)wit->second.d;
        else if (e.kind != 3 && e.param("sparse_masks", 0.0f) != 0.0f) { set_error("rle: sparse_masks is set but the last postprocess / paste left no windows"); return ISEGMI_ERR_STATE; }
    }
    void* q;
    if (h_image_hw) {
        for (int i = 0; i < N; ++i)
            if (h_image_hw[2 * i] <= 0 || h_image_hw[2 * i] > ph || h_image_hw[2 * i + 1] <= 0 || h_image_hw[2 * i + 1] > pw) { set_error("rle: image size outside the mask plane"); return ISEGMI_ERR_ARG; }
        TRY(eng_buf(e, "rle.image_hw", (int64_t)e.max_batch * 8, &q, 1, {N, 2}));
        TRY(eng_stage_small(e, h_image_hw, (size_t)N * 8, q, rs));
        a.d_image_hw = (const int32_t*)q;
    }
    int64_t tb, cb, nb, lb, eb, sb;
    TRY(isegmi_rle_workspace(N, K, ph, pw, a.cap_runs, &tb, &cb, &nb, &lb, &eb, &sb));
    TRY(eng_buf(e, "rle.ws_trans", tb, &q)); a.d_ws_trans = q;
    TRY(eng_buf(e, "rle.ws_col", cb, &q, 1)); a.d_ws_col = (int32_t*)q;
    TRY(eng_buf(e, "rle.ws_nruns", nb, &q, 1)); a.d_ws_nruns = (int32_t*)q;
    TRY(eng_buf(e, "rle.ws_tile", lb, &q, 1)); a.d_ws_tile = (int32_t*)q;
    TRY(eng_buf(e, "rle.ws_len", eb, &q, 2)); a.d_ws_len = (uint8_t*)q;
    TRY(eng_buf(e, "rle.ws_starts", sb, &q, 1)); a.d_ws_starts = (uint32_t*)q;
    TRY(eng_buf(e, "rle.run_off", ((int64_t)e.max_batch * K + 1) * 4, &q, 1, {(int64_t)N * K + 1})); a.d_out_run_off = (int32_t*)q;
    TRY(eng_buf(e, "rle.counts", (int64_t)a.cap_runs * 4, &q, 1, {a.cap_runs})); a.d_out_counts = (uint32_t*)q;
    TRY(eng_buf(e, "rle.str_off", ((int64_t)e.max_batch * K + 1) * 4, &q, 1, {(int64_t)N * K + 1})); a.d_out_str_off = (int32_t*)q;
    TRY(eng_buf(e, "rle.chars", (int64_t)a.cap_chars, &q, 2, {a.cap_chars})); a.d_out_chars = (uint8_t*)q;
    TRY(eng_buf(e, "rle.status", 16, &q, 1, {4})); a.d_out_status = (int32_t*)q;
    {
        // the chain reads each mask's box WINDOW of its uint8 plane once; the windows are data (on the device): the caller prices this stage from
        // det.mask_window (bench.py), 0 here
        OpScope op(e, rs, "rle (7 prefix-sum launches: pack, scans, emit, lengths, chars)", 0.0);
        TRY(rle_encode_launch(&a, rs));
        // Yolact's traditional NMS: the per-class capacity's flag travels in the reserved status word (0 in every other mode and engine)
        if (e.kind == 1 && e.param("nms_mode", 0.0f) == 2.0f && e.bufs.count("det.nms_overflow"))
            TRY(yolact_nms_status_launch((const int32_t*)e.bufs["det.nms_overflow"].d, N, a.d_out_status, rs));
    }
    if (rs == e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));  // reads det.masks / det.count: extend the WAR fence
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_engine_rle(isegmi_engine* h, const int32_t* h_image_hw) {
    ARG_CHECK(h, "null");
    return eng_rle(h->e, h_image_hw);
}

extern "C" int isegmi_engine_coco_record_bytes(isegmi_engine* h, int N, int64_t* bytes, int64_t* chars_offset) {
    ARG_CHECK(h && bytes && N > 0 && N <= h->e.max_batch, "record_bytes args");
    if (box_only(h->e)) {
        *bytes = maskrcnn_keypoint_on(h->e) ? keypoint_record_layout(N, det_cap(h->e), maskrcnn_num_keypoints(h->e)).total : box_record_layout(N, det_cap(h->e)).total;
        if (chars_offset) *chars_offset = *bytes;
        return ISEGMI_OK;
    }
    return record_layout(h->e, N, nullptr, chars_offset, bytes);
}

// One launch writes everything in front of the strings.  The block is laid out for `nb` image slots (nb >= the last forward's n: a short
// last batch of a data set still fills a block of the fixed per-step size); slots n .. nb-1 carry count 0 and empty strings.
struct PackK {
    const void* box; int box_elem;  // bytes per box coordinate: 4 (f32) or 8 (i64)
    const int* count; const float* score; const int* label; const float* mscore; const int* str_off; const int* status;
    int n, nb, K;
    char* dst;
    int64_t off_box, off_count, off_score, off_label, off_mscore, off_stroff;
};
__global__ void pack_coco_kernel(const PackK p) {
    const int64_t nk = (int64_t)p.n * p.K, nbk = (int64_t)p.nb * p.K;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (tid < 4) ((int*)p.dst)[tid] = p.status[tid];
    for (int64_t i = tid; i < p.nb; i += nth) ((int*)(p.dst + p.off_count))[i] = i < p.n ? p.count[i] : 0;
    const int words = p.box_elem / 4 * 4;  // 32-bit words per box
    for (int64_t i = tid; i < nbk * words; i += nth) ((uint32_t*)(p.dst + p.off_box))[i] = i < nk * words ? ((const uint32_t*)p.box)[i] : 0u;
    for (int64_t i = tid; i < nbk; i += nth) {
        ((float*)(p.dst + p.off_score))[i] = i < nk ? p.score[i] : 0.0f;
        ((int*)(p.dst + p.off_label))[i] = i < nk ? p.label[i] : 0;
        if (p.mscore) ((float*)(p.dst + p.off_mscore))[i] = i < nk ? p.mscore[i] : 0.0f;
    }
    for (int64_t i = tid; i <= nbk; i += nth) ((int*)(p.dst + p.off_stroff))[i] = p.str_off[i <= nk ? i : nk];
}

// The box-only block in one launch: boxes scaled to original-image coordinates (x * ratio_w, y * ratio_h: one fp32 multiplication each, as
// scale_boxes_kernel), counts, scores, labels; image slots n .. nb-1, the status words and the padding between sections are zero.
struct PackBoxK {
    const float* box; const float* ratios; const int* count; const float* score; const int* label;
    int n, nb, K;
    char* dst;
    BoxRecordLayout l;
};
__device__ __forceinline__ void pack_box_sections(const PackBoxK& p, int64_t tid, int64_t nth) {
    const int64_t nk = (int64_t)p.n * p.K, nbk = (int64_t)p.nb * p.K;
    if (tid < 4) ((int*)p.dst)[tid] = 0;
    for (int64_t i = tid; i < nbk; i += nth) {
        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < nk) {
            const int img = (int)(i / p.K);
            const float rw = p.ratios[2 * img], rh = p.ratios[2 * img + 1];
            const float4 s = *(const float4*)(p.box + i * 4);
            b = make_float4(s.x * rw, s.y * rh, s.z * rw, s.w * rh);
        }
        *(float4*)(p.dst + p.l.box + i * 16) = b;
    }
    // each section up to the next one's start (the padding words of an odd-sized section included)
    for (int64_t i = tid; i < (p.l.score - p.l.count) / 4; i += nth) ((int*)(p.dst + p.l.count))[i] = i < p.n ? p.count[i] : 0;
    for (int64_t i = tid; i < (p.l.label - p.l.score) / 4; i += nth) ((float*)(p.dst + p.l.score))[i] = i < nk ? p.score[i] : 0.0f;
    for (int64_t i = tid; i < (p.l.total - p.l.label) / 4; i += nth) ((int*)(p.dst + p.l.label))[i] = i < nk ? p.label[i] : 0;
}
__global__ void pack_box_records_kernel(const PackBoxK p) {
    pack_box_sections(p, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// The keypoint block in one launch: the box-only sections as above, then the keypoints -- x * ratio_w, y * ratio_h (one fp32 multiplication each, as the
// boxes), v copied -- and their logits; slots at or beyond an image's count were zeroed by keypoint_decode_kernel, slots n .. nb-1 and the padding are zero here.
struct PackKeypointK {
    PackBoxK b;
    const float* kpt; const float* kscore;
    int NK;
    int64_t off_kpt, off_kscore, total;
};
__global__ void pack_keypoint_records_kernel(const PackKeypointK p) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    pack_box_sections(p.b, tid, nth);
    const int64_t per_img = (int64_t)p.b.K * p.NK, live = (int64_t)p.b.n * per_img;
    for (int64_t i = tid; i < (p.off_kscore - p.off_kpt) / 4; i += nth) {
        float v = 0.0f;
        if (i < live * 3) {
            const int c = (int)(i % 3), img = (int)(i / (per_img * 3));
            v = p.kpt[i];
            if (c < 2) v = v * p.b.ratios[2 * img + c];
        }
        ((float*)(p.b.dst + p.off_kpt))[i] = v;
    }
    for (int64_t i = tid; i < (p.total - p.off_kscore) / 4; i += nth) ((float*)(p.b.dst + p.off_kscore))[i] = i < live ? p.kscore[i] : 0.0f;
}

// both box record forms: `keypoints` adds the kpt / kscore sections (one launch either way)
static int pack_box_family(isegmi_engine* h, const float* h_ratios_wh, void* d_dst, int64_t cap, int n_block, int64_t* bytes, bool keypoints) {
    const std::string who = keypoints ? "pack_keypoint_records" : "pack_box_records";   // the entry point that was called
    ARG_CHECK(h && h_ratios_wh && d_dst && bytes, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 2, (who + ": engine is not a Mask R-CNN / Faster R-CNN engine").c_str());
    ARG_CHECK(!keypoints || maskrcnn_keypoint_on(e), "pack_keypoint_records: the engine has no keypoint head (keypoint_on 0, MODEL.KEYPOINT_ON False)");
    const int N = e.last_N;
    ARG_CHECK(N > 0, "pack before forward");
    ARG_CHECK(n_block >= N && n_block <= e.max_batch, "n_block: between the last forward's batch and max_batch");
    const int K = det_cap(e), NK = keypoints ? maskrcnn_num_keypoints(e) : 0;
    PackKeypointK pk;
    memset(&pk, 0, sizeof(pk));
    PackBoxK& p = pk.b;
    const KeypointRecordLayout kl = keypoint_record_layout(n_block, K, NK);
    p.l = kl.b;
    const int64_t total = keypoints ? kl.total : kl.b.total;
    ARG_CHECK(total <= cap, "record buffer too small");
    const char* names[6] = {"det.box", "det.count", "det.score", "det.label", "det.kpt", "det.kscore"};
    const int64_t need[6] = {(int64_t)N * K * 16, (int64_t)N * 4, (int64_t)N * K * 4, (int64_t)N * K * 4, (int64_t)N * K * NK * 12, (int64_t)N * K * NK * 4};
    void* src[6];
    for (int i = 0; i < (keypoints ? 6 : 4); ++i) {
        auto it = e.bufs.find(names[i]);
        if (it == e.bufs.end() || it->second.d == nullptr || it->second.bytes < need[i]) { set_error(who + ": buffer not produced yet: " + names[i]); return ISEGMI_ERR_STATE; }
        src[i] = it->second.d;
    }
    hipStream_t rs = eng_results_stream(e);
    void* rt;
    TRY(maskrcnn_stage_ratios(e, h_ratios_wh, N, rs, &rt));
    p.box = (const float*)src[0]; p.count = (const int*)src[1]; p.score = (const float*)src[2]; p.label = (const int*)src[3];
    p.ratios = (const float*)rt; p.n = N; p.nb = n_block; p.K = K; p.dst = (char*)d_dst;
    if (keypoints) {
        pk.kpt = (const float*)src[4]; pk.kscore = (const float*)src[5]; pk.NK = NK;
        pk.off_kpt = kl.kpt; pk.off_kscore = kl.kscore; pk.total = kl.total;
        hipLaunchKernelGGL(pack_keypoint_records_kernel, dim3(32), dim3(256), 0, rs, pk);
    } else {
        hipLaunchKernelGGL(pack_box_records_kernel, dim3(16), dim3(256), 0, rs, p);
    }
    HIP_TRY(hipGetLastError());
    if (rs == e.tail && e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));   // reads det.*: extend the WAR fence
    *bytes = total;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_pack_box_records(isegmi_engine* h, const float* h_ratios_wh, void* d_dst, int64_t cap, int n_block, int64_t* bytes) {
    return pack_box_family(h, h_ratios_wh, d_dst, cap, n_block, bytes, false);
}

extern "C" int isegmi_engine_pack_keypoint_records(isegmi_engine* h, const float* h_ratios_wh, void* d_dst, int64_t cap, int n_block, int64_t* bytes) {
    return pack_box_family(h, h_ratios_wh, d_dst, cap, n_block, bytes, true);
}

// Keypoint R-CNN -> Pose2Seg: isegmi_op_pose_handoff over the last forward's det.* buffers on the results stream, into the caller's buffers
extern "C" int isegmi_engine_pose_handoff(isegmi_engine* h, const float* h_ratios_wh, float person_thresh, float kp_thresh, int K, float* d_kpts_out,
                                          float* d_score_out, int32_t* d_src_slot, int32_t* d_count_out) {
    ARG_CHECK(h && h_ratios_wh && d_kpts_out && d_score_out && d_src_slot && d_count_out, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 2, "pose_handoff: engine is not a Mask R-CNN-family engine");
    ARG_CHECK(maskrcnn_keypoint_on(e), "pose_handoff: the engine has no keypoint head (keypoint_on 0, MODEL.KEYPOINT_ON False)");
    const int N = e.last_N;
    ARG_CHECK(N > 0, "pose_handoff before forward");
    const int cap = det_cap(e), NK = maskrcnn_num_keypoints(e);
    const char* names[4] = {"det.score", "det.count", "det.kpt", "det.kscore"};
    const int64_t need[4] = {(int64_t)N * cap * 4, (int64_t)N * 4, (int64_t)N * cap * NK * 12, (int64_t)N * cap * NK * 4};
    void* src[4];
    for (int i = 0; i < 4; ++i) {
        auto it = e.bufs.find(names[i]);
        if (it == e.bufs.end() || it->second.d == nullptr || it->second.bytes < need[i]) { set_error(std::string("pose_handoff: buffer not produced yet: ") + names[i]); return ISEGMI_ERR_STATE; }
        src[i] = it->second.d;
    }
    hipStream_t rs = eng_results_stream(e);
    void* rt;
    TRY(maskrcnn_stage_ratios(e, h_ratios_wh, N, rs, &rt));
    {
        OpScope op(e, rs, "pose hand-off (threshold, rank, scale)", (double)N * cap * (4 + NK * 16));
        TRY(isegmi_op_pose_handoff((const float*)src[0], (const int32_t*)src[1], (const float*)src[2], (const float*)src[3], (const float*)rt, N, cap, NK,
                                   person_thresh, kp_thresh, K, d_kpts_out, d_score_out, d_src_slot, d_count_out, rs));
    }
    if (rs == e.tail && e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));   // reads det.*: extend the WAR fence
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_pack_coco_records(isegmi_engine* h, void* d_dst, int64_t cap, int n_block, int64_t* bytes) {
    ARG_CHECK(h && d_dst && bytes, "null");
    Engine& e = h->e;
    const int N = e.last_N;
    ARG_CHECK(N > 0, "pack before forward");
    ARG_CHECK(!box_only(e), "pack_coco_records carries RLE strings: a box-only engine (mask_on 0) packs with isegmi_engine_pack_box_records");
    ARG_CHECK(n_block >= N && n_block <= e.max_batch, "n_block: between the last forward's batch and max_batch");
    std::vector<Section> secs;
    int64_t coff = 0, total = 0;
    TRY(record_layout(e, n_block, &secs, &coff, &total));
    ARG_CHECK(total <= cap, "record buffer too small");
    hipStream_t rs = eng_results_stream(e);
    const int K = det_cap(e);
    const bool y = e.kind == 1;
    PackK p;
    memset(&p, 0, sizeof(p));
    p.n = N; p.nb = n_block; p.K = K; p.dst = (char*)d_dst; p.box_elem = y ? 8 : 4;
    int64_t off = 0;
    for (auto& sct : secs) {
        auto it = e.bufs.find(sct.buf);
        if (it == e.bufs.end() || it->second.d == nullptr) { set_error(std::string("pack_coco_records: buffer not produced yet: ") + sct.buf + " (run postprocess / paste and isegmi_engine_rle first)"); return ISEGMI_ERR_STATE; }
        const std::string nm = sct.buf;
        void* d = it->second.d;
        if (nm == "rle.status") p.status = (const int*)d;
        else if (nm == "det.box_int" || nm == "det.box_resized") { p.box = d; p.off_box = off; }
        else if (nm == "det.count") { p.count = (const int*)d; p.off_count = off; }
        else if (nm == "det.score") { p.score = (const float*)d; p.off_score = off; }
        else if (nm == "det.class" || nm == "det.label") { p.label = (const int*)d; p.off_label = off; }
        else if (nm == "det.mask_score") { p.mscore = (const float*)d; p.off_mscore = off; }
        else if (nm == "rle.str_off") { p.str_off = (const int*)d; p.off_stroff = off; }
        off += sct.bytes;
    }
    hipLaunchKernelGGL(pack_coco_kernel, dim3(64), dim3(256), 0, rs, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync((char*)d_dst + coff, e.bufs["rle.chars"].d, (size_t)(total - coff), hipMemcpyDeviceToDevice, rs));
    if (rs == e.tail && e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));
    *bytes = total;
    return ISEGMI_OK;
}

static int dl_init(Engine& e) {
    if (e.dl_done[0]) return ISEGMI_OK;
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&e.dl_done[i], hipEventDisableTiming));
    return ISEGMI_OK;
}

// Asynchronous D2H of `bytes` at d_src into PINNED host memory, ordered behind everything enqueued so far on the results stream; two slots so that step t+1 may produce while step t's block is still in flight:
//   download_fence(slot): later work on the results stream waits for the slot's previous download (call before overwriting its d_src);
//   download_wait(slot):  host wait, after which h_dst holds the block.
extern "C" int isegmi_engine_download_async(isegmi_engine* h, int slot, void* h_dst_pinned, const void* d_src, int64_t bytes) {
    ARG_CHECK(h && h_dst_pinned && d_src && bytes > 0 && slot >= 0 && slot < 2, "download args");
    Engine& e = h->e;
    TRY(dl_init(e));
    // The copy rides on the RESULTS stream itself, right behind the kernels that produced the block.  A download stream of its own (first
    // version) is one more stream for the runtime to fold onto its four hardware queues, and it landed on the MAIN stream's: the copy of step i --
    // enqueued after forward i, waiting for step i's last kernel -- then sat in that in-order queue in front of forward i+1's backbone, and the
    // whole cross-step overlap was gone (tools/e2e_timeline.py: backbone i+1 started 70 us after copy i; value_e2e 5 % under value at 8.3 ms
    // per step, 19 % at 2.3 ms).
    hipStream_t rs = eng_results_stream(e);
    HIP_TRY(hipMemcpyAsync(h_dst_pinned, d_src, (size_t)bytes, hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipEventRecord(e.dl_done[slot], rs));
    e.dl_used[slot] = true;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_download_fence(isegmi_engine* h, int slot) {
    ARG_CHECK(h && slot >= 0 && slot < 2, "download slot");
    Engine& e = h->e;
    if (e.dl_used[slot]) HIP_TRY(hipStreamWaitEvent(eng_results_stream(e), e.dl_done[slot], 0));
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_download_wait(isegmi_engine* h, int slot) {
    ARG_CHECK(h && slot >= 0 && slot < 2, "download slot");
    if (h->e.dl_used[slot]) HIP_TRY(hipEventSynchronize(h->e.dl_done[slot]));
    return ISEGMI_OK;
}
