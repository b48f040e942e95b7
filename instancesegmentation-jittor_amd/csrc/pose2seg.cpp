// pose2seg.cpp -- the Pose2Seg engine (model_kind 3): uint8 images + COCO keypoints -> one mask per person at the image's
// own size.  Letterbox, ResNet body, FPN down to P2 (the P3-P5 output convolutions are not run), template fit, Affine-Align, skeleton features,
// SegModule and the fused softmax + reverse warp, all on the engine's main stream.  Results land in det.masks / det.box_resized / det.score /
// det.label / det.count, so isegmi_engine_rle and isegmi_engine_pack_coco_records work as for Mask R-CNN (fp32 boxes, i32 labels).
//
// Params: max_instances (32; the record capacity K), cat_skeleton (1), align_corners (0), warp_round_u8 (1), swap_rb (0), fpn_bilinear (0 = nearest x2).
// The forward is two halves: isegmi_pose2seg_body, everything up to p2s.p2, and isegmi_pose2seg_persons, fit ... masks, which may take
// keypoints and scores another engine's stream wrote on the device; isegmi_pose2seg_forward is the two in sequence.
// fp16 and graph are refused.  Layers (isegmi_engine_set_conv, BN folded): backbone.conv1 (Cin 4), backbone.layers.L.B.{conv1,conv2,conv3,downsample.0},
// fpn.lateral2..5, fpn.output2, segnet.conv1 (Cin = the RoI tensor's channels), segnet.stage1.B.*, segnet.stage2.B.*, segnet.conv_out; tensor
// pose_templates [T][17][3] fp32.
#include <string.h>

#include <algorithm>

#include "engine.h"

namespace isegmi {

static const float kP2sMean[3] = {0.485f, 0.456f, 0.406f};
static const float kP2sStd[3] = {0.229f, 0.224f, 0.225f};

int pose2seg_det_cap(Engine& e) { return (int)e.param("max_instances", 32.0f); }

static int p2s_blocks(Engine& e, const std::string& prefix) {
    int n = 0;
    while (e.convs.count(prefix + "." + std::to_string(n) + ".conv1")) ++n;
    return n;
}

// blocks <prefix>.0 .. of torchvision bottlenecks (relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut), stride on conv2), as many as the
// weights hold; a block projects its shortcut where it has a downsample.0
static int p2s_res_stage(Engine& e, const std::string& prefix, int stride, Tensor* x) {
    ResStage rs;
    rs.layers = rs.bufs = prefix;
    rs.blocks = p2s_blocks(e, prefix);
    rs.stride = stride;
    rs.proj_by_name = true;
    return resnet_stage(e, rs, *x, x);
}

// a host array of any size through the pinned ring, slot by slot
static int p2s_stage(Engine& e, const void* h, size_t bytes, void* d) {
    for (size_t off = 0; off < bytes; off += Engine::PIN_SLOT_BYTES) {
        const size_t n = std::min(bytes - off, (size_t)Engine::PIN_SLOT_BYTES);
        TRY(eng_stage_small(e, (const char*)h + off, n, (char*)d + off, e.stream));
    }
    return ISEGMI_OK;
}

// m1 of an image in fp64 (the restatement's m1_of): into the 512 x 512 input plane, centred at the largest scale that fits
static void p2s_m1(int h, int w, double m1[6]) {
    const double s = std::min(512.0 / w, 512.0 / h);
    const double tx = 256.0 - s * w / 2.0, ty = 256.0 - s * h / 2.0;
    const double m[6] = {s, 0.0, tx, 0.0, s, ty};
    for (int i = 0; i < 6; ++i) m1[i] = m[i];
}

// The half of the forward that does not depend on the persons: per-image table, letterbox, ResNet body, FPN down to p2s.p2 (left in e.p2s_p2 / e.p2s_hw)
static int pose2seg_body(Engine& e, const uint8_t* d_u8, const int32_t* h_hw, int N) {
    const bool cat = e.param("cat_skeleton", 1.0f) != 0.0f;
    e.cur = e.stream;
    e.p2s_hw.clear();
    // per-image table of the letterbox: the inverse of m1 rounded to fp32
    std::vector<isegmi_p2s_image> table(N);
    int64_t off = 0;
    for (int n = 0; n < N; ++n) {
        const int h = h_hw[2 * n], w = h_hw[2 * n + 1];
        double m1[6];
        p2s_m1(h, w, m1);
        const double s = m1[0], tx = m1[2], ty = m1[5];
        const double mi[6] = {1.0 / s, 0.0, -tx / s, 0.0, 1.0 / s, -ty / s};
        memset(&table[n], 0, sizeof(table[n]));
        table[n].offset = off; table[n].h = h; table[n].w = w;
        for (int i = 0; i < 6; ++i) table[n].minv[i] = (float)mi[i];
        off += (int64_t)h * w * 3;
    }
    void* q;
    TRY(eng_buf(e, "p2s.table", (int64_t)e.max_batch * sizeof(isegmi_p2s_image), &q, 2));
    isegmi_p2s_image* d_table = (isegmi_p2s_image*)q;
    TRY(p2s_stage(e, table.data(), (size_t)N * sizeof(isegmi_p2s_image), d_table));
    TRY(eng_wait_upload(e, d_u8, off, e.stream));
    Tensor x4;
    TRY(eng_act(e, "p2s.input", N, 512, 512, 4, &x4));
    {
        OpScope op(e, e.stream, "pose2seg letterbox", (double)off + (double)x4.numel() * 4);
        TRY(isegmi_op_pose2seg_letterbox(d_u8, d_table, N, 512, kP2sMean, kP2sStd, (int)e.param("swap_rb", 0.0f), (int)e.param("warp_round_u8", 1.0f),
                                         x4.d, e.stream));
    }
    // ResNet body
    Tensor s, x;
    TRY(eng_conv(e, "backbone.conv1", x4, 2, 3, 1, nullptr, "p2s.stem", &s));
    TRY(eng_act(e, "p2s.pool", N, (s.H - 1) / 2 + 1, (s.W - 1) / 2 + 1, s.C, &x));
    TRY(maxpool_launch(s.d, N, s.H, s.W, s.C, 3, 2, 1, x.d, e.stream));
    Tensor feats[4];
    for (int l = 0; l < 4; ++l) {
        const std::string pre = "backbone.layers." + std::to_string(l);
        if (p2s_blocks(e, pre) == 0) { set_error("pose2seg: no blocks in " + pre + "."); return ISEGMI_ERR_STATE; }
        TRY(p2s_res_stage(e, pre, l > 0 ? 2 : 1, &x));
        feats[l] = x;
    }
    // FPN top-down to P2
    Tensor inner, lat, nxt, p2;
    TRY(eng_conv(e, "fpn.lateral5", feats[3], 1, 0, 0, nullptr, "p2s.inner5", &inner));
    const bool bil = e.param("fpn_bilinear", 0.0f) != 0.0f;
    for (int l = 2; l >= 0; --l) {
        const std::string ln = std::to_string(l + 2);
        TRY(eng_conv(e, "fpn.lateral" + ln, feats[l], 1, 0, 0, nullptr, "p2s.lat" + ln, &lat));
        TRY(eng_act(e, "p2s.inner" + ln, N, lat.H, lat.W, lat.C, &nxt));
        if (bil) TRY(resize_bilinear_launch(inner.d, N, inner.H, inner.W, inner.C, lat.H, lat.W, lat.d, 0, nxt.d, e.stream));
        else TRY(nearest2x_add_launch(inner.d, N, inner.H, inner.W, inner.C, lat.d, lat.H, lat.W, nxt.d, e.stream));
        inner = nxt;
    }
    TRY(eng_conv(e, "fpn.output2", inner, 1, 1, 0, nullptr, "p2s.p2", &p2));
    if (p2.H != 128 || p2.W != 128) { set_error("pose2seg: P2 is not 128 x 128"); return ISEGMI_ERR_STATE; }
    const int croi = cat ? p2.C + 64 : p2.C;
    auto c1 = e.convs.find("segnet.conv1");
    if (c1 == e.convs.end() || c1->second.Cin != croi) { set_error("pose2seg: segnet.conv1 must take " + std::to_string(croi) + " input channels"); return ISEGMI_ERR_STATE; }
    e.p2s_p2 = p2;
    e.p2s_hw.assign(h_hw, h_hw + 2 * N);
    return ISEGMI_OK;
}

// The half that does: template fit, Affine-Align, skeleton features, SegModule, masks -- of the batch the last pose2seg_body ran.  `producer`: the stream
// whose work so far wrote d_kpts / d_scores (the hand-off); the main stream waits for an event recorded there, which takes the place of eng_wait_upload.
static int pose2seg_persons(Engine& e, const float* d_kpts, const float* d_scores, const int32_t* h_counts, hipStream_t producer) {
    const int K = pose2seg_det_cap(e);
    const bool cat = e.param("cat_skeleton", 1.0f) != 0.0f;
    const int N = (int)(e.p2s_hw.size() / 2);
    const int32_t* h_hw = e.p2s_hw.data();
    const Tensor p2 = e.p2s_p2;
    const int croi = cat ? p2.C + 64 : p2.C;
    e.cur = e.stream;
    std::vector<double> m1s((size_t)N * 6);
    std::vector<int32_t> roi_img, roi_off(N);
    int Hmax = 0, Wmax = 0, R = 0;
    for (int n = 0; n < N; ++n) {
        p2s_m1(h_hw[2 * n], h_hw[2 * n + 1], &m1s[(size_t)n * 6]);
        Hmax = std::max(Hmax, h_hw[2 * n]); Wmax = std::max(Wmax, h_hw[2 * n + 1]);
        roi_off[n] = R;
        for (int k = 0; k < h_counts[n]; ++k) roi_img.push_back(n);
        R += h_counts[n];
    }
    void* q;
    // fit, Affine-Align, skeleton -> RoI tensor; SegModule -> logits
    const int Rb = R > 0 ? R : 1;
    float *m3, *G, *mm, *kal;
    double* fit;
    TRY(eng_buf(e, "p2s.m3", (int64_t)Rb * 24, &q, 0, {R, 6})); m3 = (float*)q;
    TRY(eng_buf(e, "p2s.G", (int64_t)Rb * 24, &q, 0, {R, 6})); G = (float*)q;
    TRY(eng_buf(e, "p2s.mmask", (int64_t)Rb * 24, &q, 0, {R, 6})); mm = (float*)q;
    TRY(eng_buf(e, "p2s.kalign", (int64_t)Rb * 204, &q, 0, {R, 17, 3})); kal = (float*)q;
    TRY(eng_buf(e, "p2s.fit", (int64_t)Rb * 64, &q, 0, {R, 8})); fit = (double*)q;
    Tensor logits;
    TRY(eng_act(e, "p2s.logits", Rb, 64, 64, 2, &logits));
    if (R > 0) {
        auto tp = e.tensors.find("pose_templates");
        if (tp == e.tensors.end() || tp->second.bytes % 204 != 0) { set_error("pose2seg: tensor pose_templates [T][17][3] not set"); return ISEGMI_ERR_STATE; }
        TRY(eng_buf(e, "p2s.roi_img", (int64_t)e.max_batch * K * 4, &q, 1));
        int32_t* d_ri = (int32_t*)q;
        TRY(p2s_stage(e, roi_img.data(), (size_t)R * 4, d_ri));
        TRY(eng_buf(e, "p2s.m1", (int64_t)e.max_batch * 48, &q));
        double* d_m1 = (double*)q;
        TRY(p2s_stage(e, m1s.data(), (size_t)N * 48, d_m1));
        if (producer) {
            hipEvent_t ev;
            TRY(eng_next_event(e, &ev));
            HIP_TRY(hipEventRecord(ev, producer));
            HIP_TRY(hipStreamWaitEvent(e.stream, ev, 0));
        } else {
            TRY(eng_wait_upload(e, d_kpts, (int64_t)R * 204, e.stream));
        }
        TRY(isegmi_op_pose2seg_fit(d_kpts, d_ri, R, d_m1, (const float*)tp->second.d, (int)(tp->second.bytes / 204), (int)e.param("align_corners", 0.0f),
                                   m3, G, mm, kal, fit, e.stream));
        Tensor roi;
        TRY(eng_act(e, "p2s.roi", R, 64, 64, croi, &roi));
        {
            OpScope op(e, e.stream, "pose2seg align + skeleton", (double)roi.numel() * 4);
            TRY(isegmi_op_pose2seg_align(p2.d, 128, 128, p2.C, d_ri, G, R, roi.d, croi, e.stream));
            if (cat) TRY(isegmi_op_pose2seg_skeleton(kal, R, roi.d, croi, p2.C, e.stream));
        }
        Tensor t, up;
        TRY(eng_conv(e, "segnet.conv1", roi, 2, 3, 1, nullptr, "p2s.seg.c1", &t));
        TRY(p2s_res_stage(e, "segnet.stage1", 1, &t));
        TRY(eng_act(e, "p2s.seg.up", R, 2 * t.H, 2 * t.W, t.C, &up));
        TRY(resize_bilinear_launch(t.d, R, t.H, t.W, t.C, up.H, up.W, nullptr, 0, up.d, e.stream));
        t = up;
        TRY(p2s_res_stage(e, "segnet.stage2", 1, &t));
        if (t.H != 64 || t.W != 64) { set_error("pose2seg: SegModule output is not 64 x 64"); return ISEGMI_ERR_STATE; }
        TRY(eng_conv(e, "segnet.conv_out", t, 1, 0, 0, nullptr, "p2s.logits", &logits));
    }
    TRY(eng_input_consumed(e));   // the last reader of the uploaded images and keypoints
    // masks at every image's own size, tight boxes, score / label / count
    void *d_cnt, *d_off, *d_hw, *masks, *boxes, *scores, *labels, *cnt_out, *ws;
    TRY(eng_buf(e, "p2s.counts", (int64_t)e.max_batch * 4, &d_cnt, 1));
    TRY(p2s_stage(e, h_counts, (size_t)N * 4, d_cnt));
    TRY(eng_buf(e, "p2s.roi_off", (int64_t)e.max_batch * 4, &d_off, 1));
    TRY(p2s_stage(e, roi_off.data(), (size_t)N * 4, d_off));
    TRY(eng_buf(e, "p2s.image_hw", (int64_t)e.max_batch * 8, &d_hw, 1, {N, 2}));
    TRY(p2s_stage(e, h_hw, (size_t)N * 8, d_hw));
    TRY(eng_buf(e, "det.masks", (int64_t)N * K * Hmax * Wmax, &masks, 2, {N, K, Hmax, Wmax}));
    TRY(eng_buf(e, "det.box_resized", (int64_t)e.max_batch * K * 16, &boxes, 0, {N, K, 4}));
    TRY(eng_buf(e, "det.score", (int64_t)e.max_batch * K * 4, &scores, 0, {N, K}));
    TRY(eng_buf(e, "det.label", (int64_t)e.max_batch * K * 4, &labels, 1, {N, K}));
    TRY(eng_buf(e, "det.count", (int64_t)e.max_batch * 4, &cnt_out, 1, {N}));
    TRY(eng_buf(e, "p2s.ws_box", (int64_t)e.max_batch * K * 16, &ws, 1));
    {
        OpScope op(e, e.stream, "pose2seg masks (softmax + reverse warp)", (double)N * K * Hmax * Wmax);
        TRY(isegmi_op_pose2seg_masks(logits.d, mm, (const int32_t*)d_cnt, (const int32_t*)d_off, (const int32_t*)d_hw, N, K, Hmax, Wmax, (int32_t*)ws,
                                     (uint8_t*)masks, (float*)boxes, (float*)scores, (int32_t*)labels, (int32_t*)cnt_out, e.stream));
    }
    if (d_scores && R > 0) TRY(isegmi_op_pose_scores(d_scores, (const int32_t*)d_cnt, N, K, (float*)scores, e.stream));
    if (producer && d_kpts) {   // the last read of the producer's buffers: what isegmi_pose2seg_wait_persons waits for
        hipEvent_t& ev = e.p2s_kpts_read[d_kpts];
        if (ev == nullptr) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, e.stream));
    }
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

static int p2s_check_body(isegmi_engine* h, const uint8_t* d_u8_staging, const int32_t* h_sizes_hw, int N) {
    ARG_CHECK(h && d_u8_staging && h_sizes_hw, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 3, "engine is not a Pose2Seg engine");
    ARG_CHECK(N > 0 && N <= e.max_batch, "batch size");
    if (e.param("fp16", 0.0f) != 0.0f || e.fp16) { set_error("pose2seg: fp16 is not supported (fp32 only)"); return ISEGMI_ERR_ARG; }
    if (e.param("graph", 0.0f) != 0.0f) { set_error("pose2seg: graph capture is not supported (graph must be 0)"); return ISEGMI_ERR_ARG; }
    const int K = pose2seg_det_cap(e);
    ARG_CHECK(K >= 1 && (int64_t)e.max_batch * K <= 65535, "max_instances");
    for (int n = 0; n < N; ++n) ARG_CHECK(h_sizes_hw[2 * n] > 0 && h_sizes_hw[2 * n + 1] > 0, "image sizes");
    return ISEGMI_OK;
}

static int p2s_check_persons(Engine& e, const float* d_kpts, const int32_t* h_counts, int N) {
    const int K = pose2seg_det_cap(e);
    int R = 0;
    for (int n = 0; n < N; ++n) {
        if (h_counts[n] < 0 || h_counts[n] > K) {
            char b[160];
            snprintf(b, sizeof(b), "pose2seg: image %d has %d persons, more than max_instances = %d", n, h_counts[n], K);
            set_error(b);
            return ISEGMI_ERR_ARG;
        }
        R += h_counts[n];
    }
    ARG_CHECK(R == 0 || d_kpts, "keypoints");
    return ISEGMI_OK;
}

extern "C" int isegmi_pose2seg_forward(isegmi_engine* h, const uint8_t* d_u8_staging, const int32_t* h_sizes_hw, const float* d_kpts,
                                       const int32_t* h_counts, int N) {
    ARG_CHECK(h_counts, "null");
    TRY(p2s_check_body(h, d_u8_staging, h_sizes_hw, N));
    Engine& e = h->e;
    TRY(p2s_check_persons(e, d_kpts, h_counts, N));
    TRY(pose2seg_body(e, d_u8_staging, h_sizes_hw, N));
    const int rc = pose2seg_persons(e, d_kpts, nullptr, h_counts, nullptr);
    e.p2s_hw.clear();   // one persons half per body
    if (rc != ISEGMI_OK) return rc;
    e.last_N = N;
    return ISEGMI_OK;
}

extern "C" int isegmi_pose2seg_body(isegmi_engine* h, const uint8_t* d_u8_staging, const int32_t* h_sizes_hw, int N) {
    TRY(p2s_check_body(h, d_u8_staging, h_sizes_hw, N));
    return pose2seg_body(h->e, d_u8_staging, h_sizes_hw, N);
}

extern "C" int isegmi_pose2seg_persons(isegmi_engine* h, const float* d_kpts, const float* d_scores, const int32_t* h_counts, void* producer_stream) {
    ARG_CHECK(h && h_counts, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 3, "engine is not a Pose2Seg engine");
    if (e.p2s_hw.empty()) { set_error("pose2seg_persons: no body of this batch: call isegmi_pose2seg_body first"); return ISEGMI_ERR_STATE; }
    const int N = (int)(e.p2s_hw.size() / 2);
    TRY(p2s_check_persons(e, d_kpts, h_counts, N));
    const int rc = pose2seg_persons(e, d_kpts, d_scores, h_counts, (hipStream_t)producer_stream);
    e.p2s_hw.clear();   // one persons half per body
    if (rc == ISEGMI_OK) e.last_N = N;
    return rc;
}

extern "C" int isegmi_pose2seg_wait_persons(isegmi_engine* h, const float* d_kpts) {
    ARG_CHECK(h && d_kpts, "null");
    auto it = h->e.p2s_kpts_read.find(d_kpts);
    if (it != h->e.p2s_kpts_read.end()) HIP_TRY(hipEventSynchronize(it->second));
    return ISEGMI_OK;
}
