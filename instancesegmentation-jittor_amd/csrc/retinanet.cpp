// retinanet.cpp -- the RetinaNet engine (model_kind 4; [UPSTREAM-RECALL] maskrcnn-benchmark retinanet_R-50/101-FPN): ResNet trunk
// (stride in the first 1x1, FrozenBN folded by the host) -> P3-P7 FPN (laterals on C3-C5, nearest top-down, LastLevelP6P7 on C5) -> RetinaNetHead, one
// set of weights over the five levels (two towers of 3x3 256 -> 256 + ReLU, cls_logits 3x3 -> A*80, bbox_pred 3x3 -> A*4) -> thresholded top-k and decode
// per (level, image) -> class-wise NMS and the detections-per-image cut (csrc/retinanet_ops.hip).  Everything runs on the engine's main stream; results
// land in det.count / det.box / det.score / det.label like the Mask R-CNN box head's.  Trunk, anchors, NMS flags, canvas checks: maskrcnn.cpp's shared stages.
//
// Every point of the graph that holds several independent convolutions is ONE grouped launch (eng_conv_group): the three laterals; the three output
// convolutions with the two evaluations of top_blocks.p6 (P6 goes on without the ReLU, P7 reads relu(P6): the small p6 convolution runs with act 0 and
// with act 1, which equals relu(conv) bit for bit); each tower layer over 5 levels x 2 towers; the two predictors over the five levels.
//
// Params: retina_pre_nms_top_n (1000, <= 1024), retina_inference_th (0.05), retina_nms_th (0.4), retina_num_convs (4), retina_levels (5: the only count
// built), detections_per_img (100), detections_cap, resnet_depth (50 / 101), nms_ge / nms_plus_one / nms_index_order.  fp16 and graph are refused.
// Layers: the trunk's, backbone.fpn.fpn_inner{2,3,4}, backbone.fpn.fpn_layer{2,3,4}, backbone.fpn.top_blocks.{p6,p7}, rpn.head.cls_tower.{0,2,..},
// rpn.head.bbox_tower.{0,2,..}, rpn.head.cls_logits, rpn.head.bbox_pred; tensors anchor_base.<l> [A][4] with params anchor_stride<l>, l = 0..4.
#include <string.h>

#include "engine.h"

namespace isegmi {

constexpr int RETINA_LEVELS = 5;

static int retina_level_hw(int H, int W, int l, int* h, int* w) {   // P3 = canvas / 8, each further level (x + 1) / 2: 3x3 stride 2 pad 1 and the halving of the trunk agree
    int a = H / 8, b = W / 8;
    for (int i = 0; i < l; ++i) { a = (a - 1) / 2 + 1; b = (b - 1) / 2 + 1; }
    *h = a; *w = b;
    return a * b;
}

static int retinanet_forward(Engine& e, const float* d_images, int N) {
    const int H = e.cur_H, W = e.cur_W, L = RETINA_LEVELS;
    const bool regen_anchors = e.anchor_H != H || e.anchor_W != W;
    e.cur = e.stream;
    hipStream_t st = e.stream;
    eng_mark(e, "start");
    Tensor C[4];
    TRY(rcnn_trunk(e, d_images, N, true, C));

    // ---- FPN: in_channels_list [0, 512, 1024, 2048] -- C2 has no lateral and no output
    Tensor lat[2], last[3], P[5], p6r;
    {
        std::vector<ConvGroupItem> g(3);
        g[0].layer = "backbone.fpn.fpn_inner2"; g[0].in = C[1]; g[0].out_name = "fpn.lat2"; g[0].out = &lat[0];
        g[1].layer = "backbone.fpn.fpn_inner3"; g[1].in = C[2]; g[1].out_name = "fpn.lat3"; g[1].out = &lat[1];
        g[2].layer = "backbone.fpn.fpn_inner4"; g[2].in = C[3]; g[2].out_name = "fpn.last4"; g[2].out = &last[2];
        TRY(eng_conv_group(e, g));
    }
    for (int l = 1; l >= 0; --l) {
        TRY(eng_act(e, "fpn.last" + std::to_string(l + 2), N, lat[l].H, lat[l].W, lat[l].C, &last[l], 0));
        TRY(nearest2x_add_launch(last[l + 1].d, N, last[l + 1].H, last[l + 1].W, last[l + 1].C, lat[l].d, lat[l].H, lat[l].W, last[l].d, st));
    }
    {
        std::vector<ConvGroupItem> g(5);
        for (int l = 0; l < 3; ++l) {
            g[l].layer = "backbone.fpn.fpn_layer" + std::to_string(l + 2); g[l].in = last[l]; g[l].pad = 1; g[l].out_name = "P" + std::to_string(l + 3); g[l].out = &P[l];
        }
        g[3].layer = "backbone.fpn.top_blocks.p6"; g[3].in = C[3]; g[3].stride = 2; g[3].pad = 1; g[3].act = 0; g[3].out_name = "P6"; g[3].out = &P[3];
        g[4] = g[3]; g[4].act = 1; g[4].out_name = "P6.relu"; g[4].out = &p6r;
        TRY(eng_conv_group(e, g));
    }
    TRY(eng_conv(e, "backbone.fpn.top_blocks.p7", p6r, 2, 1, 0, nullptr, "P7", &P[4]));
    eng_mark(e, "fpn");

    // ---- RetinaNetHead: the same weights on all five levels
    const int num_convs = (int)e.param("retina_num_convs", 4.0f);
    Tensor c[5], b[5];
    for (int l = 0; l < L; ++l) c[l] = b[l] = P[l];
    for (int i = 0; i < num_convs; ++i) {
        std::vector<ConvGroupItem> g(2 * L);
        Tensor nc[5], nb[5];
        const std::string pp = (i & 1) ? ".b" : ".a";   // a layer never writes the buffer it reads
        for (int l = 0; l < L; ++l) {
            g[l].layer = "rpn.head.cls_tower." + std::to_string(2 * i); g[l].in = c[l]; g[l].pad = 1; g[l].act = 1;
            g[l].out_name = "retina.cls_t" + std::to_string(l) + pp; g[l].out = &nc[l];
            g[L + l].layer = "rpn.head.bbox_tower." + std::to_string(2 * i); g[L + l].in = b[l]; g[L + l].pad = 1; g[L + l].act = 1;
            g[L + l].out_name = "retina.box_t" + std::to_string(l) + pp; g[L + l].out = &nb[l];
        }
        TRY(eng_conv_group(e, g));
        for (int l = 0; l < L; ++l) { c[l] = nc[l]; b[l] = nb[l]; }
    }
    Tensor logits[5], deltas[5];
    {
        std::vector<ConvGroupItem> g(2 * L);
        for (int l = 0; l < L; ++l) {
            g[l].layer = "rpn.head.cls_logits"; g[l].in = c[l]; g[l].pad = 1; g[l].out_name = "retina.logits" + std::to_string(l); g[l].out = &logits[l];
            g[L + l].layer = "rpn.head.bbox_pred"; g[L + l].in = b[l]; g[L + l].pad = 1; g[L + l].out_name = "retina.deltas" + std::to_string(l); g[L + l].out = &deltas[l];
        }
        TRY(eng_conv_group(e, g));
    }
    eng_mark(e, "head");

    // ---- the tail: selection + decode, then class-wise NMS and the cut
    auto ab = e.tensors.find("anchor_base.0");
    if (ab == e.tensors.end() || ab->second.bytes % 16) { set_error("tensor not set: anchor_base.0"); return ISEGMI_ERR_STATE; }
    const int A = (int)(ab->second.bytes / 16);
    if (deltas[0].C != 4 * A || logits[0].C % A) { set_error("retinanet: cls_logits / bbox_pred channels do not match the anchors per cell"); return ISEGMI_ERR_STATE; }
    const int nclass = logits[0].C / A;
    const int top_n = (int)e.param("retina_pre_nms_top_n", 1000.0f);
    const int dpi = (int)e.param("detections_per_img", 100), cap = maskrcnn_det_cap(e);
    isegmi_retina_select_args sa;
    memset(&sa, 0, sizeof(sa));
    sa.nl = L; sa.N = N; sa.A = A; sa.C = nclass; sa.top_n = top_n;
    sa.score_thresh = e.param("retina_inference_th", 0.05f); sa.min_size = 0.0f;
    int hw_max[RETINA_LEVELS];   // buffers are sized once, for the largest canvas and batch
    double logit_bytes = 0;
    for (int l = 0; l < L; ++l) {
        const std::string ls = std::to_string(l);
        auto base = e.tensors.find("anchor_base." + ls);
        if (base == e.tensors.end() || base->second.bytes != (int64_t)A * 16) { set_error("tensor not set (or of the wrong size): anchor_base." + ls); return ISEGMI_ERR_STATE; }
        int mh, mw;
        hw_max[l] = retina_level_hw(e.H, e.W, l, &mh, &mw);
        TRY(level_anchors(e, l, base->second, A, logits[l].H, logits[l].W, hw_max[l], regen_anchors, &sa.d_anchors[l]));
        sa.HW[l] = logits[l].H * logits[l].W;
        sa.d_logits[l] = logits[l].d; sa.d_deltas[l] = deltas[l].d;
        logit_bytes += (double)N * sa.HW[l] * A * nclass * 4;
    }
    const int64_t ws_sel = retina_select_workspace_bytes(L, e.max_batch, hw_max, A, nclass, top_n);
    const int64_t ws_post = retina_post_workspace_bytes(e.max_batch, L, top_n);
    if (ws_sel < 0 || ws_post < 0) { set_error("retinanet: retina_pre_nms_top_n must be 1..1024"); return ISEGMI_ERR_ARG; }
    void* q;
    const int64_t B = e.max_batch;
    TRY(eng_buf(e, "retina.select_ws", ws_sel, &q, 2)); sa.d_ws = q; sa.ws_bytes = ws_sel;
    TRY(eng_buf(e, "retina.sel_score", B * L * top_n * 4, &q, 0, {N, L, top_n})); sa.d_sel_scores = (float*)q;
    TRY(eng_buf(e, "retina.sel_idx", B * L * top_n * 4, &q, 1, {N, L, top_n})); sa.d_sel_idx = (int32_t*)q;
    TRY(eng_buf(e, "retina.sel_cnt", B * L * 4, &q, 1, {N, L})); sa.d_sel_cnt = (int32_t*)q;
    TRY(eng_buf(e, "retina.cand_box", B * L * top_n * 16, &q, 0, {N, L * top_n, 4})); sa.d_out_boxes = (float*)q;
    TRY(eng_buf(e, "retina.cand_score", B * L * top_n * 4, &q, 0, {N, L * top_n})); sa.d_out_scores = (float*)q;
    TRY(eng_buf(e, "retina.cand_label", B * L * top_n * 4, &q, 1, {N, L * top_n})); sa.d_out_labels = (int32_t*)q;
    TRY(eng_buf(e, "retina.cand_cnt", B * L * 4, &q, 1, {N, L})); sa.d_out_cnt = (int32_t*)q;
    sa.d_image_hw = (int*)e.last_hw_ptr;
    {   // algorithmic bytes: every logit once + deltas and anchor of the selected (32 B) + the candidate rows written (24 B)
        OpScope op(e, st, "retina_select (sigmoid + threshold + top-k + decode, all levels)", logit_bytes + (double)N * L * top_n * 56);
        TRY(retina_select_launch(&sa, st));
    }
    eng_mark(e, "select");
    isegmi_retina_post_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.N = N; pa.nseg = L; pa.seg_len = top_n; pa.ncls = nclass + 1; pa.det_per_img = dpi; pa.cap = cap; pa.nms_flags = maskrcnn_nms_flags(e);
    pa.nms_thresh = e.param("retina_nms_th", 0.4f);
    pa.d_boxes = sa.d_out_boxes; pa.d_scores = sa.d_out_scores; pa.d_labels = sa.d_out_labels; pa.d_seg_cnt = sa.d_out_cnt;
    TRY(eng_buf(e, "retina.post_ws", ws_post, &q, 2)); pa.d_ws = q; pa.ws_bytes = ws_post;
    TRY(eng_buf(e, "det.count", B * 4, &q, 1, {N})); pa.d_out_count = (int32_t*)q;
    TRY(eng_buf(e, "det.box", B * cap * 16, &q, 0, {N, cap, 4})); pa.d_out_boxes = (float*)q;
    TRY(eng_buf(e, "det.score", B * cap * 4, &q, 0, {N, cap})); pa.d_out_scores = (float*)q;
    TRY(eng_buf(e, "det.label", B * cap * 4, &q, 1, {N, cap})); pa.d_out_labels = (int32_t*)q;
    {   // candidate rows read and written once in sorted order (2 x 24 B) + the detections
        OpScope op(e, st, "retina_postprocess (class-wise NMS + detection cut)", (double)N * L * top_n * 48 + (double)N * cap * 24);
        TRY(retina_postprocess_launch(&pa, st));
    }
    eng_mark(e, "postprocess");
    e.anchor_H = H; e.anchor_W = W;
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_retinanet_forward_canvas(isegmi_engine* h, const float* d_images, const int32_t* h_image_hw, int N, int H, int W) {
    ARG_CHECK(h && d_images && h_image_hw, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 4, "engine is not a RetinaNet engine");
    TRY(rcnn_canvas_check(e, N, H, W));
    ARG_CHECK(H % 32 == 0 && W % 32 == 0, "RetinaNet input must be padded to a multiple of 32");
    if (e.param("fp16", 0.0f) != 0.0f || e.fp16) { set_error("retinanet: fp16 is not supported (fp32 only)"); return ISEGMI_ERR_ARG; }
    if (e.param("graph", 0.0f) != 0.0f) { set_error("retinanet: graph capture is not supported (graph must be 0)"); return ISEGMI_ERR_ARG; }
    if ((int)e.param("retina_levels", 5.0f) != RETINA_LEVELS) { set_error("retinanet: retina_levels must be 5 (P3-P7 is the only pyramid built)"); return ISEGMI_ERR_ARG; }
    const int top_n = (int)e.param("retina_pre_nms_top_n", 1000.0f);
    if (top_n < 1 || top_n > 1024) { set_error("retinanet: retina_pre_nms_top_n must be 1..1024 (what the selection kernels hold)"); return ISEGMI_ERR_ARG; }
    if ((int)e.param("retina_num_convs", 4.0f) < 1) { set_error("retinanet: retina_num_convs must be at least 1"); return ISEGMI_ERR_ARG; }
    TRY(rcnn_begin_canvas(e, d_images, h_image_hw, N, H, W));
    const int rc = retinanet_forward(e, d_images, N);
    e.cur = e.stream;
    if (rc == ISEGMI_OK) e.last_N = N;
    return rc;
}

extern "C" int isegmi_retinanet_forward(isegmi_engine* h, const float* d_images, const int32_t* h_image_hw, int N) {
    ARG_CHECK(h, "null");
    return isegmi_retinanet_forward_canvas(h, d_images, h_image_hw, N, h->e.H, h->e.W);
}
