// yolov3.cpp -- the YOLOv3 engine (model_kind 5; [UPSTREAM-RECALL] the public yolov3.cfg, unverified): Darknet-53 (darknet.cpp) ->
// three heads, s = 0 at stride 32: head.<s>.conv0..4 (1x1 -> M, 3x3 -> 2M, 1x1, 3x3, 1x1; M = 512 / 256 / 128), conv5 (3x3 -> 2M), conv6 (1x1 -> 3 (5 + C), bias,
// linear); for s = 1, 2 the input is concat(up2x(head.<s>.route(conv4 of head s - 1)), trunk map), the upsampled half first (route layers = -1, 61) ->
// yolo_select -> class-wise NMS and the detections-per-image cut of retina_postprocess (csrc/yolo_ops.hip, csrc/retinanet_ops.hip).  Every convolution
// with BN is conv + folded BN + LeakyReLU(0.1) (act 3).  Everything runs on the engine's main stream; results land in det.count / det.box / det.score /
// det.label in canvas coordinates.
//
// Params: yolo_conf_thresh (0.5), yolo_nms_thresh (0.4), yolo_pre_nms_top_n (1024, 1..1024), yolo_multi_label (1), yolo_min_wh (0), detections_per_img (100),
// detections_cap, nms_ge / nms_plus_one (the host sets 0: plain areas) / nms_index_order; yolo_anchor0..17 = the anchors [3][3][2] in pixels, stride 32 first.  fp16 and graph are refused.
//
// Variants ([UPSTREAM-RECALL] the public yolov3-spp.cfg / yolov3-tiny.cfg): yolo_variant 0 (default) the graph above; 1 yolov3-spp:
// head 0 is conv0, conv1, conv2, spp_concat (2048 channels), head.0.spp (1x1 -> 512), conv3 .. conv6; 2 yolov3-tiny: darknet_tiny_backbone, head.0.conv0
// (1x1 1024 -> 256, the branch), conv1 (3x3 -> 512), conv2 (predictor); head.1.route (1x1 -> 128), concat_up2x with the stride-16 map (384), head.1.conv0
// (3x3 -> 256), conv1 (predictor): two levels, strides 32 and 16, yolo_anchor0..11.  yolo_pool_zero_pad (0): 1 lets the out-of-range taps of the variants'
// max-pools count as 0 (csrc/yolo_pool.hip).  Both are read at every forward.
#include <string.h>

#include "engine.h"

namespace isegmi {

constexpr int YOLO_LEVELS = 3, YOLO_A = 3;   // YOLO_LEVELS: the most a variant has

// yolov3 (spp 0) and yolov3-spp (spp 1): Darknet-53 and three heads; spp puts spp_concat and head.0.spp (1x1 2048 -> 512) between conv2 and conv3 of head 0
static int yolov3_heads(Engine& e, const float* d_images, int N, bool spp, int zero_pad, Tensor* head) {
    hipStream_t st = e.stream;
    Tensor C[3];
    TRY(darknet_backbone(e, "backbone.", d_images, N, C, nullptr));

    Tensor x = C[2];
    for (int s = 0; s < YOLO_LEVELS; ++s) {
        const std::string hn = "head." + std::to_string(s);
        Tensor t = x, u;
        for (int i = 0; i < 5; ++i) {
            TRY(eng_conv(e, hn + ".conv" + std::to_string(i), t, 1, i & 1, 3, nullptr, hn + ".t" + std::to_string(i), &u));
            t = u;
            if (spp && s == 0 && i == 2) {
                Tensor cat;
                TRY(eng_act(e, "head.0.spp_cat", N, t.H, t.W, 4 * t.C, &cat));
                {
                    OpScope op(e, st, "spp_concat (max-pool 5 / 9 / 13 + route)", 5.0 * (double)t.numel() * 4);
                    TRY(spp_concat_launch(t.d, N, t.H, t.W, t.C, zero_pad, cat.d, st));
                }
                TRY(eng_conv(e, "head.0.spp", cat, 1, 0, 3, nullptr, "head.0.spp", &u));
                t = u;
            }
        }
        const Tensor branch = t;   // conv4's output: the predictor pair and the next head's route both read it
        TRY(eng_conv(e, hn + ".conv5", branch, 1, 1, 3, nullptr, hn + ".t5", &u));
        TRY(eng_conv(e, hn + ".conv6", u, 1, 0, 0, nullptr, "yolo.head" + std::to_string(s), &head[s]));
        if (s + 1 < YOLO_LEVELS) {
            const std::string nn = "head." + std::to_string(s + 1);
            const Tensor& skip = C[1 - s];
            Tensor r;
            TRY(eng_conv(e, nn + ".route", branch, 1, 0, 3, nullptr, nn + ".route", &r));
            if (skip.H != 2 * r.H || skip.W != 2 * r.W) { set_error("yolov3: the trunk map is not twice the routed map (canvas sides must be multiples of 32)"); return ISEGMI_ERR_STATE; }
            TRY(eng_act(e, nn + ".cat", N, skip.H, skip.W, r.C + skip.C, &x));
            OpScope op(e, st, "concat_up2x (upsample + route)", 2.0 * (double)x.numel() * 4);
            TRY(concat_up2x_launch(r.d, N, r.H, r.W, r.C, skip.d, skip.C, x.d, st));
        }
    }
    return ISEGMI_OK;
}

// yolov3-tiny: the seven-convolution trunk (darknet.cpp) and two heads.  head.0.conv0 (1x1 -> 256) is the branch; head 1 reads
// concat(up2x(head.1.route(branch)), the trunk's stride-16 map), the upsampled half first (route layers = -1, 8)
static int yolov3_tiny_heads(Engine& e, const float* d_images, int N, int zero_pad, Tensor* head) {
    hipStream_t st = e.stream;
    Tensor skip, top, branch, u, r, x;
    TRY(darknet_tiny_backbone(e, "backbone.", d_images, N, zero_pad, &skip, &top));
    TRY(eng_conv(e, "head.0.conv0", top, 1, 0, 3, nullptr, "head.0.t0", &branch));
    TRY(eng_conv(e, "head.0.conv1", branch, 1, 1, 3, nullptr, "head.0.t1", &u));
    TRY(eng_conv(e, "head.0.conv2", u, 1, 0, 0, nullptr, "yolo.head0", &head[0]));
    TRY(eng_conv(e, "head.1.route", branch, 1, 0, 3, nullptr, "head.1.route", &r));
    if (skip.H != 2 * r.H || skip.W != 2 * r.W) { set_error("yolov3: the trunk map is not twice the routed map (canvas sides must be multiples of 32)"); return ISEGMI_ERR_STATE; }
    TRY(eng_act(e, "head.1.cat", N, skip.H, skip.W, r.C + skip.C, &x));
    {
        OpScope op(e, st, "concat_up2x (upsample + route)", 2.0 * (double)x.numel() * 4);
        TRY(concat_up2x_launch(r.d, N, r.H, r.W, r.C, skip.d, skip.C, x.d, st));
    }
    TRY(eng_conv(e, "head.1.conv0", x, 1, 1, 3, nullptr, "head.1.t0", &u));
    TRY(eng_conv(e, "head.1.conv1", u, 1, 0, 0, nullptr, "yolo.head1", &head[1]));
    return ISEGMI_OK;
}

static int yolov3_forward(Engine& e, const float* d_images, int N, int variant) {
    e.cur = e.stream;
    hipStream_t st = e.stream;
    eng_mark(e, "start");
    const int L = variant == 2 ? 2 : YOLO_LEVELS;
    const int zero_pad = e.param("yolo_pool_zero_pad", 0.0f) != 0.0f ? 1 : 0;
    Tensor head[YOLO_LEVELS];
    if (variant == 2) TRY(yolov3_tiny_heads(e, d_images, N, zero_pad, head));
    else TRY(yolov3_heads(e, d_images, N, variant == 1, zero_pad, head));
    eng_mark(e, "heads");

    // ---- the tail
    if (head[0].C % YOLO_A || head[0].C / YOLO_A < 6 || head[1].C != head[0].C || head[L - 1].C != head[0].C) {
        set_error("yolov3: the predictors (head.<s>.conv6; tiny: head.0.conv2, head.1.conv1) must have 3 * (5 + classes) output channels, the same on every head");
        return ISEGMI_ERR_STATE;
    }
    const int nclass = head[0].C / YOLO_A - 5;
    const int top_n = (int)e.param("yolo_pre_nms_top_n", 1024.0f);
    const int dpi = (int)e.param("detections_per_img", 100), cap = maskrcnn_det_cap(e);
    int grid[YOLO_LEVELS * 2], grid_max[YOLO_LEVELS * 2], strides[YOLO_LEVELS] = {32, 16, 8};
    const float* heads[YOLO_LEVELS];
    float anchors[YOLO_LEVELS * YOLO_A * 2];
    for (int i = 0; i < L * YOLO_A * 2; ++i) {
        const std::string k = "yolo_anchor" + std::to_string(i);
        if (e.params.count(k) == 0 || !(e.params[k] > 0.0f)) { set_error("parameter not set (or not positive): " + k); return ISEGMI_ERR_STATE; }
        anchors[i] = e.params[k];
    }
    double head_bytes = 0;
    for (int l = 0; l < L; ++l) {
        grid[2 * l] = head[l].H; grid[2 * l + 1] = head[l].W;
        grid_max[2 * l] = e.H / strides[l]; grid_max[2 * l + 1] = e.W / strides[l];
        heads[l] = head[l].d;
        head_bytes += (double)head[l].numel() * 4;
    }
    const int64_t ws_sel = yolo_select_workspace_bytes(L, e.max_batch, grid_max, YOLO_A, nclass, top_n);
    const int64_t ws_post = retina_post_workspace_bytes(e.max_batch, L, top_n);
    if (ws_sel < 0 || ws_post < 0) { set_error("yolov3: yolo_pre_nms_top_n must be 1..1024 and the classes 1..256"); return ISEGMI_ERR_ARG; }
    void* q;
    const int64_t B = e.max_batch;
    float *cb, *cs; int32_t *cl, *cc, *ct;
    TRY(eng_buf(e, "yolo.select_ws", ws_sel, &q, 2)); void* ws = q;
    TRY(eng_buf(e, "yolo.cand_box", B * L * top_n * 16, &q, 0, {N, L * top_n, 4})); cb = (float*)q;
    TRY(eng_buf(e, "yolo.cand_score", B * L * top_n * 4, &q, 0, {N, L * top_n})); cs = (float*)q;
    TRY(eng_buf(e, "yolo.cand_label", B * L * top_n * 4, &q, 1, {N, L * top_n})); cl = (int32_t*)q;
    TRY(eng_buf(e, "yolo.cand_cnt", B * L * 4, &q, 1, {N, L})); cc = (int32_t*)q;
    TRY(eng_buf(e, "yolo.cand_total", B * L * 4, &q, 1, {N, L})); ct = (int32_t*)q;
    {   // algorithmic bytes: every head float once + the box parameters of the selected (16 B) + the candidate rows written (24 B)
        OpScope op(e, st, "yolo_select (objectness x class + threshold + top-k + decode, all levels)", head_bytes + (double)N * L * top_n * 40);
        TRY(yolo_select_launch(L, N, heads, grid, strides, anchors, YOLO_A, nclass, top_n, e.param("yolo_conf_thresh", 0.5f),
                               e.param("yolo_multi_label", 1.0f) != 0.0f ? 1 : 0, e.param("yolo_min_wh", 0.0f), e.W, e.H, ws, ws_sel, cb, cs, cl, cc, ct, st));
    }
    eng_mark(e, "select");
    isegmi_retina_post_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.N = N; pa.nseg = L; pa.seg_len = top_n; pa.ncls = nclass + 1; pa.det_per_img = dpi; pa.cap = cap; pa.nms_flags = maskrcnn_nms_flags(e);
    pa.nms_thresh = e.param("yolo_nms_thresh", 0.4f);
    pa.d_boxes = cb; pa.d_scores = cs; pa.d_labels = cl; pa.d_seg_cnt = cc;
    TRY(eng_buf(e, "yolo.post_ws", ws_post, &q, 2)); pa.d_ws = q; pa.ws_bytes = ws_post;
    TRY(eng_buf(e, "det.count", B * 4, &q, 1, {N})); pa.d_out_count = (int32_t*)q;
    TRY(eng_buf(e, "det.box", B * cap * 16, &q, 0, {N, cap, 4})); pa.d_out_boxes = (float*)q;
    TRY(eng_buf(e, "det.score", B * cap * 4, &q, 0, {N, cap})); pa.d_out_scores = (float*)q;
    TRY(eng_buf(e, "det.label", B * cap * 4, &q, 1, {N, cap})); pa.d_out_labels = (int32_t*)q;
    {
        OpScope op(e, st, "retina_postprocess (class-wise NMS + detection cut)", (double)N * L * top_n * 48 + (double)N * cap * 24);
        TRY(retina_postprocess_launch(&pa, st));
    }
    eng_mark(e, "post");
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_yolov3_forward(isegmi_engine* h, const float* d_images, int N) {
    ARG_CHECK(h && d_images, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 5, "engine is not a YOLOv3 engine");
    ARG_CHECK(N > 0 && N <= e.max_batch, "batch size");
    const float variant = e.param("yolo_variant", 0.0f), zp = e.param("yolo_pool_zero_pad", 0.0f);
    if (variant != 0.0f && variant != 1.0f && variant != 2.0f) { set_error("yolov3: yolo_variant must be 0 (yolov3), 1 (yolov3-spp) or 2 (yolov3-tiny)"); return ISEGMI_ERR_ARG; }
    if (zp != 0.0f && zp != 1.0f) { set_error("yolov3: yolo_pool_zero_pad must be 0 (out-of-range taps ignored) or 1 (they count as 0)"); return ISEGMI_ERR_ARG; }
    if (variant == 2.0f && e.params.count("yolo_anchor12")) {
        set_error("yolov3: yolo_anchor12 is set, but yolo_variant 2 (yolov3-tiny) has two levels: its anchors are yolo_anchor0..11");
        return ISEGMI_ERR_ARG;
    }
    if (e.param("fp16", 0.0f) != 0.0f || e.fp16) { set_error("yolov3: fp16 is not supported (fp32 only)"); return ISEGMI_ERR_ARG; }
    if (e.param("graph", 0.0f) != 0.0f) { set_error("yolov3: graph capture is not supported (graph must be 0)"); return ISEGMI_ERR_ARG; }
    const int top_n = (int)e.param("yolo_pre_nms_top_n", 1024.0f);
    if (top_n < 1 || top_n > 1024) { set_error("yolov3: yolo_pre_nms_top_n must be 1..1024 (what the selection kernels hold)"); return ISEGMI_ERR_ARG; }
    const float ct = e.param("yolo_conf_thresh", 0.5f), nt = e.param("yolo_nms_thresh", 0.4f), mw = e.param("yolo_min_wh", 0.0f);
    if (!(ct >= 0.0f)) { set_error("yolov3: yolo_conf_thresh must be a non-negative number"); return ISEGMI_ERR_ARG; }
    if (!(nt > 0.0f)) { set_error("yolov3: yolo_nms_thresh must be positive"); return ISEGMI_ERR_ARG; }
    if (!(mw >= 0.0f)) { set_error("yolov3: yolo_min_wh must be a non-negative number"); return ISEGMI_ERR_ARG; }
    TRY(eng_wait_upload(e, d_images, (int64_t)N * e.H * e.W * 3 * 4, e.stream));
    const int rc = yolov3_forward(e, d_images, N, (int)variant);
    e.cur = e.stream;
    if (rc == ISEGMI_OK) e.last_N = N;
    return rc;
}
