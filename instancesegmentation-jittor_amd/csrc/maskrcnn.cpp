// maskrcnn.cpp -- Mask R-CNN R50/R101-FPN forward graph.
//
// GeneralizedRCNN: ResNet (stride in the first 1x1, FrozenBN folded by the host) -> FPN (nearest
// top-down, no activation, P6 = P5[::2,::2]) -> RPN head (shared 3x3 + fused 1x1 cls|bbox) ->
// per-level top-k/decode/clip/NMS -> per-image top-1000 -> RoIAlign 7x7 -> FC6/FC7/predictors ->
// per-class NMS + kth-value cut -> RoIAlign 14x14 on detections -> 4x conv3x3 -> deconv2x2 (as four
// strided 1x1 convolutions) -> class-selected 1x1 + sigmoid.  Reached from
// COCODemo.run_on_opencv_image (README.md:331) and tools/test_net.py (README.md:344-347).
//
// Built from stages.  Shared with retinanet.cpp (engine.h): rcnn_trunk, maskrcnn_nms_flags, level_anchors, rcnn_canvas_check / rcnn_begin_canvas.
// maskrcnn_forward (FPN): rcnn_trunk -> fpn_topdown_grouped | fpn_topdown_levels -> fpn_out_and_rpn (fpn_out_grouped | fpn_out_levels with rpn_level,
// rpn_select_group, the hand-over to the tail stream) -> merge_proposals -> box_head (roi_pool, 2-FC | Xconv1fc) -> box_tail -> keypoint_head | mask_head
// (roi_pool each), passing one RcnnCtx.  maskrcnn_c4_forward: rcnn_trunk (plain form), its single-map RPN, the conv5 head and box_tail, on one stream.
#include <string.h>

#include "engine.h"

namespace isegmi {

// SURVEY 7.2 / App. A.6-A.7 semantic forks as engine parameters (defaults = the maskrcnn-benchmark CUDA path): "nms_ge" 1 suppress on iou >= thr;
// "nms_plus_one" 0 plain areas in the NMS IoU; "nms_index_order" 1 a class's detections in ascending proposal index (CPU nonzero order);
// "roi_aligned" 1 ROIAlign(aligned=True).
int maskrcnn_nms_flags(Engine& e) {
    return ((int)e.param("nms_ge", 0) ? ISEGMI_NMS_GE : 0) | ((int)e.param("nms_plus_one", 1) ? 0 : ISEGMI_NMS_NO_PLUS_ONE) |
           ((int)e.param("nms_index_order", 0) ? ISEGMI_NMS_INDEX_ORDER : 0);
}

static int need_tensor(Engine& e, const std::string& name, int64_t bytes, const RawBuf** out) {
    auto it = e.tensors.find(name);
    if (it == e.tensors.end()) { set_error("tensor not set: " + name); return ISEGMI_ERR_STATE; }
    if (bytes > 0 && it->second.bytes != bytes) { set_error("tensor " + name + " has the wrong size"); return ISEGMI_ERR_STATE; }
    *out = &it->second;
    return ISEGMI_OK;
}

// image_hw is caller memory and changes from batch to batch on real data: it reaches the device through the pinned ring (asynchronous
// copy on the main stream) into one of TWO device buffers used alternately -- the previous forward's RoI heads (tail stream) may still
// read theirs; the one before that finished before the previous forward's WAR wait on tail_done, which precedes this copy in stream
// order.  Kept out of maskrcnn_forward so that the forward's enqueue code is capturable into a hipGraph.
int maskrcnn_set_image_hw(Engine& e, const int32_t* h_image_hw, int N) {
    std::vector<int32_t> now(h_image_hw, h_image_hw + 2 * N);
    if (now == e.last_hw && e.last_hw_ptr != nullptr) return ISEGMI_OK;  // steady-state batches: the current buffer already holds it
    e.hw_slot ^= 1;
    void* p;
    TRY(eng_buf(e, e.hw_slot ? "image_hw.1" : "image_hw.0", (int64_t)e.max_batch * 8, &p, 1, {N, 2}));
    TRY(eng_stage_small(e, h_image_hw, (size_t)N * 8, p, e.stream));
    e.last_hw = now;
    e.last_hw_ptr = p;
    return ISEGMI_OK;
}

// The canvas entry points' checks (Mask R-CNN and RetinaNet): the batch and the canvas fit the engine ...
int rcnn_canvas_check(Engine& e, int N, int H, int W) {
    ARG_CHECK(N > 0 && N <= e.max_batch, "batch size");
    ARG_CHECK(H > 0 && W > 0 && H <= e.H && W <= e.W, "canvas must fit inside the engine's maximum input size");
    return ISEGMI_OK;
}

// ... and every image fits the canvas; then the forward's inputs: the main stream behind the upload, image_hw on the device, the current canvas
int rcnn_begin_canvas(Engine& e, const float* d_images, const int32_t* h_image_hw, int N, int H, int W) {
    for (int i = 0; i < N; ++i)
        ARG_CHECK(h_image_hw[2 * i] > 0 && h_image_hw[2 * i] <= H && h_image_hw[2 * i + 1] > 0 && h_image_hw[2 * i + 1] <= W,
                  "image_hw must fit inside the padded canvas");
    TRY(eng_wait_upload(e, d_images, (int64_t)N * H * W * 3 * 4, e.stream));
    TRY(maskrcnn_set_image_hw(e, h_image_hw, N));
    e.cur_H = H; e.cur_W = W;
    return ISEGMI_OK;
}

// the GroupNorm behind a convolution, where the layer has one (gn_baselines: MODEL.FPN.USE_GN, ROI_BOX_HEAD.USE_GN, ROI_MASK_HEAD.USE_GN)
static int gn_after(Engine& e, const std::string& layer, Tensor* x, bool relu) {
    return eng_has_gn(e, layer) ? eng_gn(e, layer, x, nullptr, relu) : ISEGMI_OK;
}

// rows of every per-image detection buffer: DETECTIONS_PER_IMG, or more when "detections_cap" is set -- upstream's kth-value rule keeps every
// detection whose score ties with the 100th, so an image can return more than DETECTIONS_PER_IMG; the extra rows hold those ties
int maskrcnn_det_cap(Engine& e) {
    const int dpi = (int)e.param("detections_per_img", 100);
    const int cap = (int)e.param("detections_cap", 0.0f);
    return cap > dpi ? cap : dpi;
}

// MODEL.MASK_ON: "mask_on" 0 = Faster R-CNN -- the forward ends behind box_postprocess, no mask buffer is ever allocated, the results leave
// through isegmi_engine_pack_box_records.  Read each forward: an engine whose weights include the mask head may be toggled.
bool maskrcnn_mask_on(Engine& e) { return e.param("mask_on", 1.0f) != 0.0f; }

// MODEL.KEYPOINT_ON: "keypoint_on" 1 = Keypoint R-CNN -- behind box_postprocess the keypoint head runs over the detections and the results
// leave through isegmi_engine_pack_keypoint_records.  Built on the FrozenBN FPN bodies in fp32, next to no mask head.
bool maskrcnn_keypoint_on(Engine& e) { return e.param("keypoint_on", 0.0f) != 0.0f; }
int maskrcnn_num_keypoints(Engine& e) { return (int)e.param("num_keypoints", 17.0f); }

static int keypoint_refusals(Engine& e) {
    if (!maskrcnn_keypoint_on(e)) return ISEGMI_OK;
    const char* why = maskrcnn_mask_on(e) ? "mask_on 1 (MODEL.MASK_ON True): a model with both heads is not built, set mask_on 0"
                      : e.fp16 ? "fp16: the keypoint head is fp32 only"
                      : e.param("arch_c4", 0.0f) != 0.0f ? "arch_c4 (the R-50-C4 body): the keypoint head reads P2..P5"
                      : eng_has_gn(e, "backbone.body.stem.conv1") ? "GroupNorm weights (USE_GN): the keypoint head is built on the FrozenBN bodies"
                      : nullptr;
    if (why) { set_error(std::string("keypoint_on 1 (MODEL.KEYPOINT_ON) together with ") + why); return ISEGMI_ERR_STATE; }
    const int nk = maskrcnn_num_keypoints(e);
    if (nk < 1 || nk > 32) { set_error("num_keypoints (MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES) must be 1..32, got " + std::to_string(nk)); return ISEGMI_ERR_STATE; }
    return ISEGMI_OK;
}

// The box predictor's shape: "num_classes" (MODEL.ROI_BOX_HEAD.NUM_CLASSES, background included) and "cls_agnostic" (MODEL.CLS_AGNOSTIC_BBOX_REG: two
// sets of four deltas, the last one decoded for every class).  `width` = outputs of the fused cls_score | bbox_pred layer.
static int box_predictor_shape(Engine& e, int width, int* ncls, int* agnostic) {
    const int nc = (int)e.param("num_classes", 81.0f), ag = e.param("cls_agnostic", 0.0f) != 0.0f ? 1 : 0;
    if (nc < 2 || nc > 257) { set_error("num_classes (MODEL.ROI_BOX_HEAD.NUM_CLASSES) must be 2..257, got " + std::to_string(nc)); return ISEGMI_ERR_STATE; }
    const int want = ag ? nc + 8 : nc * 5;
    if (width != want) {
        set_error("cls_bbox layer has " + std::to_string(width) + " outputs; " + std::to_string(nc) + " classes need " +
                  (ag ? std::to_string(nc) + "+8 (class-agnostic regression: cls_agnostic 1)" : std::to_string(nc) + "+" + std::to_string(4 * nc) + " (per-class regression: cls_agnostic 0)"));
        return ISEGMI_ERR_STATE;
    }
    *ncls = nc; *agnostic = ag;
    return ISEGMI_OK;
}

// ---- stages shared by the FPN, C4 and RetinaNet graphs
// The FPN-body trunk on the current canvas: resnet_stem on backbone.body.stem.conv1, then the backbone.body.layer<l> stages; C[l] = stage l's output.
// full (FPN Mask R-CNN, RetinaNet): four stages in the full form, "resnet_depth" and "stride_in_1x1" from the parameters (MODEL.RESNETS.STRIDE_IN_1X1 is
// False in the GroupNorm yaml), the marks stem, res2..res5.  Otherwise (C4) the plain form -- one stream, one buffer per layer: three stages of
// {3, 4, 6} blocks, the stride in the 1x1, no marks.
int rcnn_trunk(Engine& e, const float* d_images, int N, bool full, Tensor* C) {
    static const char* const stages[4] = {"res2", "res3", "res4", "res5"};
    Tensor x;
    TRY(resnet_stem(e, "backbone.body.stem.conv1", d_images, N, e.cur_H, e.cur_W, &x));
    if (full) eng_mark(e, "stem");
    const int blocks[4] = {3, 4, full && (int)e.param("resnet_depth", 50) == 101 ? 23 : 6, 3};
    for (int li = 0; li < (full ? 4 : 3); ++li) {
        ResStage rs;
        rs.layers = rs.bufs = "backbone.body.layer" + std::to_string(li + 1);
        rs.blocks = blocks[li];
        rs.stride = li > 0 ? 2 : 1;
        rs.stride_in_1x1 = !full || e.param("stride_in_1x1", 1.0f) != 0.0f;
        rs.full = full; rs.stage = stages[li];   // (the plain form names no stage buffers)
        TRY(resnet_stage(e, rs, x, &x));
        C[li] = x;
        if (full) eng_mark(e, stages[li]);
    }
    return ISEGMI_OK;
}

// Anchors of one level for the current canvas: the host sets the A base anchors (`base` = the tensor "anchor_base.<l>", generate_anchors; the caller
// looks it up and words its absence) and the stride ("anchor_stride<l>"); the gh x gw grid is laid out on the device, in a buffer of cap_cells cells,
// whenever the caller says so -- when the canvas changed, and in Mask R-CNN always under graph capture, so that a replayed graph never depends on which
// canvas ran last.  Runs on the main stream, after the forward's WAR wait on the previous forward's tail.
int level_anchors(Engine& e, int l, const RawBuf& base, int A, int gh, int gw, int64_t cap_cells, bool regen, const float** out) {
    const std::string ls = std::to_string(l);
    const int stride = (int)e.param("anchor_stride" + ls, 0.0f);
    if (stride <= 0) { set_error("anchor_stride" + ls + " not set"); return ISEGMI_ERR_STATE; }
    void* q;
    TRY(eng_buf(e, "anchors." + ls, cap_cells * A * 16, &q, 0, {(int64_t)gh * gw * A, 4}));
    if (regen) TRY(grid_anchors_launch((const float*)base.d, A, stride, gh, gw, (float*)q, e.stream));
    *out = (const float*)q;
    return ISEGMI_OK;
}

// ---- the FPN graph by stage; what the stages hand on:
struct RcnnCtx {
    Engine& e;
    int N, dt;                 // dt: storage type of everything after the stem, 0 fp32, 1 fp16
    bool grp;                  // the FPN's and the RPN head's convolutions as grouped launches (below)
    const int* d_hw;           // image sizes on the device (maskrcnn_set_image_hw)
    int nms_flags, roi_aligned, roi_table;
    Tensor C[4], last[4], P[5];   // trunk outputs, top-down sums, P2..P6 (level sizes in P[l].H / .W)
    // RPN: configuration, the levels' candidate lists, and per level what the selection reads
    static constexpr int A = 3, CH = 15, L = 5;
    int pre_nms, post_nms, fpn_post, sel_groups;
    float rpn_thr, rpn_min;
    float *cand_boxes, *cand_scores; int *cand_cnt, *cand_total;
    const float* lvl_head[5]; const float* lvl_anc[5]; int lvl_hwa[5];
    float* props; int* prop_cnt;   // merge_proposals: fpn_post rows per image
    isegmi_box_post_args a;        // box_tail
};

// ---- FPN top-down chain (main stream); leaves (3x3 output convs) and the RPN follow per level
// fp32 (round 5): the four lateral convs, the four output convs, the RPN head's 3x3 over the five levels and its cls + bbox 1x1 over the five levels are
// ONE grouped launch each (eng_conv_group; bit-identical to the separate launches): 18 launches become 4, the small levels run inside the big levels'
// launches.  Needs the batched RPN selection (which then takes all five levels at once); "conv_groups" 0 restores the per-level launches.
static int fpn_topdown_grouped(RcnnCtx& x) {
    Engine& e = x.e;
    Tensor lats[3];
    std::vector<ConvGroupItem> g(4);
    g[0].layer = "backbone.fpn.fpn_inner1"; g[0].in = x.C[0]; g[0].out_name = "fpn.lat1"; g[0].out = &lats[0];
    g[1].layer = "backbone.fpn.fpn_inner2"; g[1].in = x.C[1]; g[1].out_name = "fpn.lat2"; g[1].out = &lats[1];
    g[2].layer = "backbone.fpn.fpn_inner3"; g[2].in = x.C[2]; g[2].out_name = "fpn.lat3"; g[2].out = &lats[2];
    g[3].layer = "backbone.fpn.fpn_inner4"; g[3].in = x.C[3]; g[3].out_name = "fpn.last4"; g[3].out = &x.last[3];
    TRY(eng_conv_group(e, g));
    for (int l = 0; l < 4; ++l) TRY(gn_after(e, g[l].layer, l < 3 ? &lats[l] : &x.last[3], false));   // the top-down add consumes the normalised lateral
    for (int l = 2; l >= 0; --l) {
        const Tensor& up = x.last[l + 1];
        TRY(eng_act(e, "fpn.last" + std::to_string(l + 1), x.N, lats[l].H, lats[l].W, lats[l].C, &x.last[l], 0));
        TRY(nearest2x_add_launch(up.d, x.N, up.H, up.W, up.C, lats[l].d, lats[l].H, lats[l].W, x.last[l].d, e.cur));
    }
    return ISEGMI_OK;
}

static int fpn_topdown_levels(RcnnCtx& x) {
    Engine& e = x.e;
    Tensor lat;
    TRY(eng_conv(e, "backbone.fpn.fpn_inner4", x.C[3], 1, 0, 0, nullptr, "fpn.last4", &x.last[3]));
    TRY(gn_after(e, "backbone.fpn.fpn_inner4", &x.last[3], false));
    for (int l = 2; l >= 0; --l) {
        const std::string ls = std::to_string(l + 1);
        const Tensor& up = x.last[l + 1];
        if (x.dt) {  // fp16: the merge with the coarser level in the lateral conv's own epilogue (one launch, the lateral tensor never exists)
            bool merged = false;
            TRY(eng_conv_up2x_f16(e, "backbone.fpn.fpn_inner" + ls, x.C[l], up, "fpn.last" + ls, &x.last[l], &merged));
            if (merged) continue;
        }
        TRY(eng_conv(e, "backbone.fpn.fpn_inner" + ls, x.C[l], 1, 0, 0, nullptr, "fpn.lat" + ls, &lat));
        TRY(gn_after(e, "backbone.fpn.fpn_inner" + ls, &lat, false));
        TRY(eng_act(e, "fpn.last" + ls, x.N, lat.H, lat.W, lat.C, &x.last[l], x.dt));
        if (x.dt) TRY(nearest2x_add_f16_launch(up.d, x.N, up.H, up.W, up.C, lat.d, lat.H, lat.W, x.last[l].d, e.cur));
        else TRY(nearest2x_add_launch(up.d, x.N, up.H, up.W, up.C, lat.d, lat.H, lat.W, x.last[l].d, e.cur));
    }
    return ISEGMI_OK;
}

// ---- RPN config
// Per level, finest first: FPN output conv -> RPN head convs on the main stream, then that level's
// selection (sigmoid, top-k, decode, NMS: small latency-bound grids) on a side stream so it hides under the
// next level's convolutions.  P2's selection (201 600 anchors) gets all the remaining levels to hide under.
// SELECTION BATCHED OVER (level, image) (round 5; SURVEY 2.1 "level x image as ONE batch dimension"): the levels' sigmoid, pre-NMS top-k, suppression
// matrix and greedy scan run as five launches per GROUP of levels instead of four or five per level (22 launches, 520 us of latency-bound grids per
// bs = 2 step).  Batches of two or more: one group of all five levels on the tail stream behind the last head conv (it hides under the next forward's
// backbone anyway).  One image (latency): P2 -- 201 600 anchors, the longest chain -- goes first on a side stream under the other levels' convolutions,
// P3..P6 as one group behind P6's head.  "rpn_select_groups": 0 = the per-level launches (A/B; also taken for pre_nms outside 257..1024), 1 / 2 force.
static void rpn_config(RcnnCtx& x) {
    Engine& e = x.e;
    x.pre_nms = (int)e.param("rpn_pre_nms_top_n", 1000); x.post_nms = (int)e.param("rpn_post_nms_top_n", 1000);
    x.fpn_post = (int)e.param("rpn_fpn_post_nms_top_n", 1000);
    x.rpn_thr = e.param("rpn_nms_thresh", 0.7f); x.rpn_min = e.param("rpn_min_size", 0.0f);
    const int sel_groups_param = (int)e.param("rpn_select_groups", -1.0f);
    const bool batched_sel = sel_groups_param != 0 && x.pre_nms > 256 && x.pre_nms <= 1024 && x.post_nms > 0;
    x.grp = !x.dt && e.param("conv_groups", 1.0f) != 0.0f && e.param("conv_tile", 0) == 0.0f && batched_sel;
    x.sel_groups = !batched_sel ? 0 : x.grp ? 1 : (sel_groups_param > 0 ? (sel_groups_param > 2 ? 2 : sel_groups_param) : (x.N >= 2 ? 1 : 2));
}

static int rpn_select_group(RcnnCtx& x, int l0, int l1) {   // levels [l0, l1) on e.cur
    Engine& e = x.e;
    const int nl = l1 - l0, N = x.N;
    const std::string gs = std::to_string(l0) + "_" + std::to_string(l1);
    int slot[5];
    for (int l = l0; l < l1; ++l) slot[l - l0] = l;
    int64_t pe = 0, ce = 0;
    TRY(rpn_levels_workspace(nl, N, x.lvl_hwa + l0, x.pre_nms, &pe, &ce));
    void* q;
    float *prob, *cv, *tkv; int *ci, *tki, *tkc; void* nws;
    TRY(eng_buf(e, "rpn.g_prob" + gs, pe * 4, &q)); prob = (float*)q;
    TRY(eng_buf(e, "rpn.g_cand_vals" + gs, ce * 4, &q)); cv = (float*)q;
    TRY(eng_buf(e, "rpn.g_cand_idx" + gs, ce * 4, &q, 1)); ci = (int*)q;
    TRY(eng_buf(e, "rpn.g_tk_vals" + gs, (int64_t)nl * N * x.pre_nms * 4, &q)); tkv = (float*)q;
    TRY(eng_buf(e, "rpn.g_tk_idx" + gs, (int64_t)nl * N * x.pre_nms * 4, &q, 1)); tki = (int*)q;
    TRY(eng_buf(e, "rpn.g_tk_cnt" + gs, (int64_t)nl * N * 4, &q, 1)); tkc = (int*)q;
    TRY(eng_buf(e, "rpn.g_nms_ws" + gs, (int64_t)nl * N * 131072, &nws, 1));
    double bytes = 0;   // SURVEY 8d, as for the per-level form: logits once + deltas and anchors of the pre-NMS top-k + the kept boxes and scores
    for (int l = l0; l < l1; ++l) bytes += (double)N * ((double)x.lvl_hwa[l] * 4 + (double)(x.pre_nms < x.lvl_hwa[l] ? x.pre_nms : x.lvl_hwa[l]) * 32 + (double)x.post_nms * 20);
    OpScope op(e, e.cur, "rpn_select (sigmoid + top-k + decode + NMS, per FPN level)", bytes);
    return rpn_levels_select_launch(nl, x.lvl_head + l0, x.lvl_anc + l0, x.lvl_hwa + l0, slot, x.d_hw, N, x.A, x.CH, x.pre_nms, x.post_nms, x.rpn_thr, x.rpn_min,
                                    x.nms_flags, x.L, x.post_nms, prob, cv, ci, tkv, tki, tkc, nws, x.cand_boxes, x.cand_scores, x.cand_cnt, e.cur);
}

// what the selection reads of level l: the head's output and the level's anchors (a buffer of the current grid's size)
static int rpn_level_inputs(RcnnCtx& x, int l, const Tensor& head) {
    Engine& e = x.e;
    const bool regen = e.capturing || e.anchor_H != e.cur_H || e.anchor_W != e.cur_W;
    const RawBuf* base;
    TRY(need_tensor(e, "anchor_base." + std::to_string(l), (int64_t)x.A * 16, &base));
    TRY(level_anchors(e, l, *base, x.A, head.H, head.W, (int64_t)head.H * head.W, regen, &x.lvl_anc[l]));
    x.lvl_head[l] = head.d; x.lvl_hwa[l] = head.H * head.W * x.A;
    return ISEGMI_OK;
}

// the per-level selection ("rpn_select_groups" 0): three launches for level l, on the tail stream or on side stream l % 3
static int rpn_level_select(RcnnCtx& x, int l, const Tensor& head) {
    Engine& e = x.e;
    const std::string ls = std::to_string(l);
    const int N = x.N, HWA = x.lvl_hwa[l], pre_nms = x.pre_nms, post_nms = x.post_nms;
    float *prob, *tkv; int *tki, *tkc; void* q;
    TRY(eng_buf(e, "rpn.prob" + ls, (int64_t)N * HWA * 4, &q)); prob = (float*)q;
    TRY(eng_buf(e, "rpn.tk_vals" + ls, (int64_t)N * pre_nms * 4, &q)); tkv = (float*)q;
    TRY(eng_buf(e, "rpn.tk_idx" + ls, (int64_t)N * pre_nms * 4, &q, 1)); tki = (int*)q;
    TRY(eng_buf(e, "rpn.tk_cnt" + ls, (int64_t)N * 4, &q, 1)); tkc = (int*)q;
    void* nms_ws = nullptr;  // suppression matrix of the chip-wide NMS (one per level: the levels run concurrently)
    if (pre_nms <= 1024) TRY(eng_buf(e, "rpn.nms_ws" + ls, (int64_t)N * 131072, &nms_ws, 1));
    // candidate buffers of the two-level top-k (long rows): engine-owned, one pair per level (the levels run concurrently)
    float* tws_v = nullptr; int* tws_i = nullptr;
    if (const int64_t we = topk_scratch_elems(N, HWA, pre_nms)) {
        TRY(eng_buf(e, "rpn.tk_ws_vals" + ls, we * 4, &q)); tws_v = (float*)q;
        TRY(eng_buf(e, "rpn.tk_ws_idx" + ls, we * 4, &q, 1)); tws_i = (int*)q;
    }
    auto select = [&]() -> int {
        // logits once (4 B per anchor) + deltas and anchors of the pre-NMS top-k (16 B each) + the kept boxes and scores (20 B)
        OpScope op(e, e.cur, "rpn_select (sigmoid + top-k + decode + NMS, per FPN level)",
                   (double)N * ((double)HWA * 4 + (double)(pre_nms < HWA ? pre_nms : HWA) * 32 + (double)post_nms * 20));
        TRY(rpn_sigmoid_launch(head.d, (int64_t)N * HWA, x.A, x.CH, prob, e.cur));
        TRY(topk_launch_ws(prob, HWA, N, HWA, pre_nms, nullptr, 1, tkv, tki, tkc, tws_v, tws_i, e.cur));
        TRY(rpn_decode_nms_launch(head.d, x.lvl_anc[l], tkv, tki, tkc, x.d_hw, N, HWA, x.A, x.CH, pre_nms, post_nms, x.rpn_thr, x.rpn_min,
                                  x.nms_flags, l, x.L, post_nms, x.cand_boxes, x.cand_scores, x.cand_cnt, nms_ws, e.cur));
        return ISEGMI_OK;
    };
    // Batches of two or more (throughput): the level's selection goes straight to the TAIL stream, which is idle here (the main stream waited for the
    // previous forward's RoI heads before the FPN output convs) and takes everything after the RPN convs anyway; the five levels' chains then run one
    // after the other under the remaining RPN convs and the next forward's backbone.  One image (latency): on three side streams, level l on stream
    // l % 3, in parallel.  Fewer busy streams = fewer collisions on the runtime's four in-order hardware queues: +0.8 % R50 fp32 bs=2, +1.1 % R101 fp16
    // bs=8, +2.1 % R50 fp16 bs=2; bs=1 p50 5.62 -> 5.79 ms if forced there (profiles/r03_experiments.txt 3e).  "rpn_select_on_tail": 1 / 0 force.
    const float sel_tail = e.param("rpn_select_on_tail", -1.0f);
    if (e.multi_stream && !e.capturing && (sel_tail < 0.0f ? N >= 2 : sel_tail != 0.0f)) {
        hipEvent_t ev;
        TRY(eng_next_event(e, &ev));
        HIP_TRY(hipEventRecord(ev, e.cur));
        HIP_TRY(hipStreamWaitEvent(e.tail, ev, 0));
        hipStream_t saved = e.cur;
        e.cur = e.tail;
        const int rc = select();
        e.cur = saved;
        return rc;
    }
    TRY(eng_fork(e, l % 3));
    SideScope sc(e, l % 3);
    return select();
}

// level l behind its output conv, per-level form: the RPN head's convolutions, then whatever of the selection starts here
static int rpn_level(RcnnCtx& x, int l) {
    Engine& e = x.e;
    const std::string ls = std::to_string(l);
    Tensor t, head;
    bool head_fused = false;   // fp16, big levels: the 3x3 and the fused cls + bbox 1x1 in one launch, t stays in LDS
    if (x.dt) TRY(eng_rpn_head_f16(e, "rpn.head.conv", "rpn.head.cls_bbox", x.P[l], "rpn.head" + ls, &head, &head_fused));
    if (!head_fused) {
        TRY(eng_conv(e, "rpn.head.conv", x.P[l], 1, 1, 1, nullptr, "rpn.t" + ls, &t));
        TRY(eng_conv(e, "rpn.head.cls_bbox", t, 1, 0, 0, nullptr, "rpn.head" + ls, &head, /*out_f32=*/true));
    }
    TRY(rpn_level_inputs(x, l, head));
    if (x.sel_groups == 0) return rpn_level_select(x, l, head);
    if (x.sel_groups == 1 || l != 0) return ISEGMI_OK;   // all five levels as one group on the tail stream, or P3..P6 as one group behind P6's head
    if (e.multi_stream && !e.capturing) {                // P2: its own group, now, under the remaining levels' convolutions
        TRY(eng_fork(e, 0));
        SideScope sc(e, 0);
        return rpn_select_group(x, 0, 1);
    }
    return rpn_select_group(x, 0, 1);
}

static int fpn_out_grouped(RcnnCtx& x) {
    Engine& e = x.e;
    Tensor* P = x.P;
    std::vector<ConvGroupItem> g(4), gt(5), gh(5);
    for (int l = 0; l < 4; ++l) {
        g[l].layer = "backbone.fpn.fpn_layer" + std::to_string(l + 1); g[l].in = x.last[l]; g[l].pad = 1; g[l].out_name = "P" + std::to_string(l + 2); g[l].out = &P[l];
    }
    TRY(eng_conv_group(e, g));
    for (int l = 0; l < 4; ++l) TRY(gn_after(e, g[l].layer, &P[l], false));
    const int Ho = (P[3].H - 1) / 2 + 1, Wo = (P[3].W - 1) / 2 + 1;
    TRY(eng_act(e, "P6", x.N, Ho, Wo, P[3].C, &P[4], 0));
    TRY(maxpool_launch(P[3].d, x.N, P[3].H, P[3].W, P[3].C, 1, 2, 0, P[4].d, e.cur));
    Tensor t[5], head[5];
    for (int l = 0; l < 5; ++l) {
        gt[l].layer = "rpn.head.conv"; gt[l].in = P[l]; gt[l].pad = 1; gt[l].act = 1; gt[l].out_name = "rpn.t" + std::to_string(l); gt[l].out = &t[l];
    }
    TRY(eng_conv_group(e, gt));
    for (int l = 0; l < 5; ++l) {
        gh[l].layer = "rpn.head.cls_bbox"; gh[l].in = t[l]; gh[l].out_name = "rpn.head" + std::to_string(l); gh[l].out = &head[l]; gh[l].out_f32 = true;
    }
    TRY(eng_conv_group(e, gh));
    for (int l = 0; l < 5; ++l) TRY(rpn_level_inputs(x, l, head[l]));
    return ISEGMI_OK;
}

static int fpn_out_levels(RcnnCtx& x) {
    Engine& e = x.e;
    Tensor* P = x.P;
    for (int l = 0; l < 4; ++l) {
        TRY(eng_conv(e, "backbone.fpn.fpn_layer" + std::to_string(l + 1), x.last[l], 1, 1, 0, nullptr, "P" + std::to_string(l + 2), &P[l]));
        TRY(gn_after(e, "backbone.fpn.fpn_layer" + std::to_string(l + 1), &P[l], false));
        TRY(rpn_level(x, l));
    }
    const int Ho = (P[3].H - 1) / 2 + 1, Wo = (P[3].W - 1) / 2 + 1;
    TRY(eng_act(e, "P6", x.N, Ho, Wo, P[3].C, &P[4], x.dt));
    if (x.dt) TRY(maxpool_to_f16_launch(P[3].d, 1, x.N, P[3].H, P[3].W, P[3].C, 1, 2, 0, P[4].d, e.cur));
    else TRY(maxpool_launch(P[3].d, x.N, P[3].H, P[3].W, P[3].C, 1, 2, 0, P[4].d, e.cur));
    return rpn_level(x, 4);
}

static int fpn_out_and_rpn(RcnnCtx& x) {
    Engine& e = x.e;
    const int N = x.N, L = x.L;
    // per level up to 6144 (above 1024 the single-block NMS with 96 KB of boxes in LDS takes over from the chip-wide bitmask NMS); the merged
    // list feeds the per-class box NMS, whose suppression matrix holds 1024 proposals per image
    if (x.pre_nms > 6144 || x.post_nms > 6144 || x.fpn_post > 1024) { set_error("RPN: PRE / POST_NMS_TOP_N_TEST <= 6144 per level, FPN_POST_NMS_TOP_N_TEST <= 1024"); return ISEGMI_ERR_ARG; }
    void* p;
    TRY(eng_buf(e, "rpn.cand_boxes", (int64_t)N * L * x.post_nms * 16, &p, 0, {N, L * x.post_nms, 4})); x.cand_boxes = (float*)p;
    TRY(eng_buf(e, "rpn.cand_scores", (int64_t)N * L * x.post_nms * 4, &p, 0, {N, L * x.post_nms})); x.cand_scores = (float*)p;
    TRY(eng_buf(e, "rpn.cand_cnt", (int64_t)N * L * 4, &p, 1, {N, L})); x.cand_cnt = (int*)p;
    TRY(eng_buf(e, "rpn.cand_total", (int64_t)N * 4, &p, 1, {N})); x.cand_total = (int*)p;
    // WAR: the previous forward's RoI heads (tail stream) still gather from P2..P5 and read proposals / det buffers;
    // everything up to here (backbone, top-down chain) was free to run underneath them.
    if (e.multi_stream && e.tail_pending && !e.capturing) HIP_TRY(hipStreamWaitEvent(e.stream, e.tail_done, 0));
    TRY(x.grp ? fpn_out_grouped(x) : fpn_out_levels(x));
    e.anchor_H = e.cur_H; e.anchor_W = e.cur_W;
    // From here on everything runs on the TAIL stream: it (not the main stream) joins the side streams, so the main
    // stream is free the moment its last RPN convolution is queued and the next forward's backbone starts underneath
    // the remaining per-level selection kernels, proposal merge and RoI heads (all latency-bound or small grids).
    if (e.multi_stream) {
        hipStream_t srcs[4] = {e.stream, e.side[0], e.side[1], e.side[2]};
        for (int i = 0; i < 4; ++i) {
            hipEvent_t ev;
            TRY(eng_next_event(e, &ev));
            HIP_TRY(hipEventRecord(ev, srcs[i]));
            HIP_TRY(hipStreamWaitEvent(e.tail, ev, 0));
        }
        e.cur = e.tail;
    }
    if (x.sel_groups) TRY(rpn_select_group(x, x.sel_groups == 1 ? 0 : 1, L));
    return ISEGMI_OK;
}

static int merge_proposals(RcnnCtx& x) {
    Engine& e = x.e;
    const int N = x.N, L = x.L, R = x.fpn_post;
    TRY(sum_counts_launch(x.cand_cnt, N, L, x.cand_total, e.cur));
    float *fin_vals, *prop_scores; int *fin_idx, *fin_cnt; void* p;
    TRY(eng_buf(e, "rpn.fin_vals", (int64_t)N * R * 4, &p)); fin_vals = (float*)p;
    TRY(eng_buf(e, "rpn.fin_idx", (int64_t)N * R * 4, &p, 1)); fin_idx = (int*)p;
    TRY(eng_buf(e, "rpn.fin_cnt", (int64_t)N * 4, &p, 1)); fin_cnt = (int*)p;
    TRY(eng_buf(e, "proposals", (int64_t)N * R * 16, &p, 0, {N, R, 4})); x.props = (float*)p;
    TRY(eng_buf(e, "proposal_scores", (int64_t)N * R * 4, &p, 0, {N, R})); prop_scores = (float*)p;
    TRY(eng_buf(e, "proposal_count", (int64_t)N * 4, &p, 1, {N})); x.prop_cnt = (int*)p;
    OpScope op(e, e.cur, "rpn_merge (top-k over the levels' candidates + gather)", (double)N * ((double)L * x.post_nms * 4 + (double)R * 40));
    TRY(topk_launch(x.cand_scores, (int64_t)L * x.post_nms, N, L * x.post_nms, R, x.cand_total, 1, fin_vals, fin_idx, fin_cnt, e.cur));
    return gather_proposals_launch(x.cand_boxes, fin_vals, fin_idx, fin_cnt, N, L * x.post_nms, R, x.props, prop_scores, x.prop_cnt, e.cur);
}

// RoIAlign of K RoI slots per image (`rois`, counts[n] live) over P2..P5 into <prefix>.roi_feat [N * K, ph, ph, 256] of storage type dt, under one OpScope
// `label` (a literal).  `table` -- the head's "roi_table" bit (0 box head, 1 mask / keypoint head), up to 2048 rows per image: roi_prep (per-RoI sample
// table + launch order) and the table-driven channel-slice launch instead of one workgroup per RoI in proposal order (same bits; A/B).  Same-box A/B,
// profiles/r05_experiments.txt 10: the box head gains in both dtypes; the mask head's N x 100 RoIs gain in fp16 (125 -> 79 us) and lose the prep launch's
// time in fp32 (43 -> 52 us): default 3 fp16, 1 fp32.
static int roi_pool(RcnnCtx& x, const char* label, const std::string& prefix, const float* rois, const int* counts, int K, int ph, bool table, int dt, Tensor* out) {
    Engine& e = x.e;
    const int N = x.N, es = dt ? 2 : 4;
    const float* feats[4] = {x.P[0].d, x.P[1].d, x.P[2].d, x.P[3].d};
    const int Hs[4] = {x.P[0].H, x.P[1].H, x.P[2].H, x.P[3].H}, Ws[4] = {x.P[0].W, x.P[1].W, x.P[2].W, x.P[3].W};
    const float scales[4] = {0.25f, 0.125f, 0.0625f, 0.03125f};
    TRY(eng_act(e, prefix + ".roi_feat", N * K, ph, ph, 256, out, dt));
    // SURVEY 8d "RoIAlign box: read rois + P2-P5 once (compulsory) + write the pooled features"
    double bytes = (double)N * K * 20 + (double)N * K * ph * ph * 256 * es;
    for (int l = 0; l < 4; ++l) bytes += (double)N * Hs[l] * Ws[l] * 256 * es;
    OpScope op(e, e.cur, label, bytes);   // (roi_prep is launched inside the stage's scope: its time counts against the same algorithmic bytes)
    int* order = nullptr;
    void *tab = nullptr, *p;
    if (table && K <= 2048) {
        const int rows = ph == 7 ? 29 : 57;   // the box head's order buffer carries no prefix
        TRY(eng_buf(e, prefix == "box" ? "roi_order" : prefix + ".roi_order", (int64_t)N * K * 4, &p, 1, {N, K}));
        order = (int*)p;
        TRY(eng_buf(e, prefix + ".roi_table", (int64_t)N * K * rows * 16, &tab, 1, {N * K, rows, 4}));
        TRY(roi_prep_launch(rois, counts, N, K, Hs, Ws, scales, 4, 2, 256, ph, ph, es, order, tab, e.cur, x.roi_aligned));
    }
    if (dt) return roi_align_f16_launch((const void* const*)feats, Hs, Ws, scales, 4, rois, counts, N, K, 256, ph, ph, 2, 2, out->d, e.cur, order, tab, x.roi_aligned);
    return roi_align_launch(feats, Hs, Ws, scales, 4, rois, counts, N, K, 256, ph, ph, 2, 2, -1, out->d, nullptr, e.cur, order, tab, x.roi_aligned);
}

// ---- box head: RoIAlign 7x7 on the proposals -> 2-FC or Xconv1fc -> the fused predictors (*cb)
static int box_head(RcnnCtx& x, Tensor* cb) {
    Engine& e = x.e;
    Tensor roi7, f6, f7;
    TRY(roi_pool(x, "roi_align 7x7 (box head)", "box", x.props, x.prop_cnt, x.fpn_post, 7, x.roi_table & 1, x.dt, &roi7));
    if (e.convs.count("roi_heads.box.feature_extractor.xconvs.0")) {
        // FPNXconv1fcFeatureExtractor (gn_baselines): NUM_STACKED_CONVS x [3x3 conv (no bias) -> GN -> ReLU] on the 7x7 RoI features, then ReLU(fc6); no fc7
        Tensor xc = roi7;
        for (int i = 0; e.convs.count("roi_heads.box.feature_extractor.xconvs." + std::to_string(i)); ++i) {
            const std::string nm = "roi_heads.box.feature_extractor.xconvs." + std::to_string(i);
            const bool gn = eng_has_gn(e, nm);
            Tensor o;
            TRY(eng_conv(e, nm, xc, 1, 1, gn ? 0 : 1, nullptr, "box.xconv" + std::to_string(i), &o));
            TRY(gn_after(e, nm, &o, true));
            xc = o;
        }
        TRY(eng_conv(e, "roi_heads.box.feature_extractor.fc6", xc, 1, 0, 1, nullptr, "box.fc6", &f7));
    } else {
        TRY(eng_conv(e, "roi_heads.box.feature_extractor.fc6", roi7, 1, 0, 1, nullptr, "box.fc6", &f6));
        TRY(eng_conv(e, "roi_heads.box.feature_extractor.fc7", f6, 1, 0, 1, nullptr, "box.fc7", &f7));
    }
    return eng_conv(e, "roi_heads.box.predictor.cls_bbox", f7, 1, 0, 0, nullptr, "box.cls_bbox", cb, /*out_f32=*/true);
}

// The box tail on e.cur, everything from the predictor's shape to box_postprocess: argument block, workspaces, det.* outputs.  cb = the fused
// cls_score | bbox_pred rows of the N x R proposals.  *a = the filled block: the heads read d_out_boxes, d_out_count and d_out_labels from it.
static int box_tail(Engine& e, int N, int R, const Tensor& cb, const float* props, const int* prop_cnt, const int* d_hw, int nms_flags, isegmi_box_post_args* out) {
    isegmi_box_post_args& a = *out;
    void* p;
    memset(&a, 0, sizeof(a));
    TRY(box_predictor_shape(e, cb.C, &a.ncls, &a.cls_agnostic));
    const int ncls = a.ncls, dpi = (int)e.param("detections_per_img", 100), cap = maskrcnn_det_cap(e);
    a.N = N; a.R = R; a.det_per_img = dpi; a.cap = cap; a.nms_flags = nms_flags;
    a.score_thresh = e.param("roi_score_thresh", 0.05f);
    a.nms_thresh = e.param("roi_nms_thresh", 0.5f);
    a.logits_stride = cb.C; a.regr_stride = cb.C;
    a.d_logits = cb.d; a.d_regr = cb.d + ncls; a.d_props = props; a.d_prop_cnt = prop_cnt; a.d_image_hw = d_hw;
    TRY(eng_buf(e, "box.prob", (int64_t)N * R * ncls * 4, &p, 0, {N, R, ncls})); a.d_ws_prob = (float*)p;
    TRY(eng_buf(e, "box.cand_scores", (int64_t)N * (ncls - 1) * R * 4, &p)); a.d_ws_cand_scores = (float*)p;
    TRY(eng_buf(e, "box.cand_boxes", (int64_t)N * (ncls - 1) * R * 16, &p)); a.d_ws_cand_boxes = (float*)p;
    TRY(eng_buf(e, "box.kept_total", (int64_t)N * 4, &p, 1, {N})); a.d_ws_kept_total = (int*)p;
    TRY(eng_buf(e, "box.top_vals", (int64_t)N * dpi * 4, &p)); a.d_ws_top_vals = (float*)p;
    TRY(eng_buf(e, "box.top_idx", (int64_t)N * dpi * 4, &p, 1)); a.d_ws_top_idx = (int*)p;
    if ((int)e.param("box_nms_chip_wide", 1)) {   // crowded classes: suppression matrix on the whole chip (rcnn_ops.hip BoxCrowd); 0 = every class in its own block (A/B)
        TRY(eng_buf(e, "box.crowd_matrix", (int64_t)N * (ncls - 1) * 131072, &p, 1)); a.d_ws_crowd_matrix = p;
        TRY(eng_buf(e, "box.crowd_keys", (int64_t)N * (ncls - 1) * R * 8, &p, 1)); a.d_ws_crowd_keys = p;
        TRY(eng_buf(e, "box.crowd_boxes", (int64_t)N * (ncls - 1) * R * 16, &p)); a.d_ws_crowd_boxes = (float*)p;
        TRY(eng_buf(e, "box.crowd_m", (int64_t)N * (ncls - 1) * 4, &p, 1)); a.d_ws_crowd_m = (int*)p;
    }
    TRY(eng_buf(e, "det.count", (int64_t)N * 4, &p, 1, {N})); a.d_out_count = (int*)p;
    TRY(eng_buf(e, "det.box", (int64_t)N * cap * 16, &p, 0, {N, cap, 4})); a.d_out_boxes = (float*)p;
    TRY(eng_buf(e, "det.score", (int64_t)N * cap * 4, &p, 0, {N, cap})); a.d_out_scores = (float*)p;
    TRY(eng_buf(e, "det.label", (int64_t)N * cap * 4, &p, 1, {N, cap})); a.d_out_labels = (int*)p;
    // logits + box regressions of every proposal once, the proposals, the detections out
    OpScope op(e, e.cur, "box_postprocess (softmax + decode + per-class NMS + top-100)", (double)N * R * ((double)cb.C * 4 + 16) + (double)N * cap * 24);
    return box_postprocess_launch(&a, e.cur);
}

// ---- keypoint head: RoIAlign 14x14 on the detections -> conv_fcn1.. (3x3 + ReLU) -> ConvTranspose2d(4, 2, 1) as ONE 3x3 convolution
// with 4 * K parity-major outputs -> pixel shuffle + bilinear x2 -> fused bicubic resize + arg-max per (detection, keypoint)
static int keypoint_head(RcnnCtx& x) {
    Engine& e = x.e;
    const int N = x.N, cap = x.a.cap, NK = maskrcnn_num_keypoints(e);
    Tensor kf, low, heat;
    TRY(roi_pool(x, "roi_align 14x14 (keypoint head)", "kp", x.a.d_out_boxes, x.a.d_out_count, cap, 14, x.roi_table & 2, 0, &kf));
    for (int i = 1; e.convs.count("roi_heads.keypoint.feature_extractor.conv_fcn" + std::to_string(i)); ++i) {
        Tensor o;
        TRY(eng_conv(e, "roi_heads.keypoint.feature_extractor.conv_fcn" + std::to_string(i), kf, 1, 1, 1, nullptr, "kp.fcn" + std::to_string(i), &o));
        kf = o;
    }
    TRY(eng_conv(e, "roi_heads.keypoint.predictor.kps_score_lowres", kf, 1, 1, 0, nullptr, "kp.lowres68", &low, /*out_f32=*/true));
    if (low.C != 4 * NK) { set_error("kps_score_lowres has " + std::to_string(low.C) + " packed outputs; num_keypoints " + std::to_string(NK) + " needs 4 * " + std::to_string(NK)); return ISEGMI_ERR_STATE; }
    TRY(eng_act(e, "kp.heat", N * cap, 56, 56, NK, &heat));
    void *kq, *ks;
    TRY(eng_buf(e, "det.kpt", (int64_t)N * cap * NK * 12, &kq, 0, {N, cap, NK, 3}));
    TRY(eng_buf(e, "det.kscore", (int64_t)N * cap * NK * 4, &ks, 0, {N, cap, NK}));
    {
        OpScope op(e, e.cur, "keypoint_heatmap (pixel shuffle + bilinear x2)", (double)N * cap * (196.0 * 4 + 3136.0) * NK * 4);
        TRY(keypoint_heatmap_launch(low.d, (int64_t)N * cap, 14, 14, NK, heat.d, e.cur));
    }
    {
        OpScope op(e, e.cur, "keypoint_decode (bicubic resize to the box + arg-max)", (double)N * cap * NK * (3136.0 + 4) * 4);
        TRY(keypoint_decode_launch(heat.d, x.a.d_out_boxes, x.a.d_out_count, N, cap, 56, NK, (float*)kq, (float*)ks, e.cur));
    }
    eng_mark(e, "keypoint_head");
    return ISEGMI_OK;
}

// ---- mask head: RoIAlign 14x14 on the detections -> 4 x (3x3 [+ GN] + ReLU) -> deconv 2x2 -> the label's logit + sigmoid
static int mask_head(RcnnCtx& x) {
    Engine& e = x.e;
    const int N = x.N, cap = x.a.cap, dt = x.dt;
    Tensor m, up;
    TRY(roi_pool(x, "roi_align 14x14 (mask head)", "mask", x.a.d_out_boxes, x.a.d_out_count, cap, 14, x.roi_table & 2, dt, &m));
    for (int i = 1; i <= 4; ++i) {
        Tensor o;
        const std::string nm = "roi_heads.mask.feature_extractor.mask_fcn" + std::to_string(i);
        const bool gn = eng_has_gn(e, nm);
        TRY(eng_conv(e, nm, m, 1, 1, gn ? 0 : 1, nullptr, "mask.fcn" + std::to_string(i), &o));
        TRY(gn_after(e, nm, &o, true));
        m = o;
    }
    TRY(eng_act(e, "mask.deconv", N * cap, 28, 28, 256, &up, dt));
    {
        // ConvTranspose2d(2,2,s2): out[r, 2i+a, 2j+b, :] = W_ab * in[r, i, j, :] + bias  -> four strided 1x1 convs.
        Tensor rows;  // view: (r, i) as "images" of 1 x 14 pixels
        rows.d = m.d; rows.N = N * cap * 14; rows.H = 1; rows.W = 14; rows.C = 256; rows.dt = dt;
        std::vector<ConvGroupItem> g(4);   // the four parities are independent: one grouped launch under fp32 (eng_conv_group), four launches under fp16
        for (int ab = 0; ab < 4; ++ab) {
            const int aa = ab >> 1, bb = ab & 1;
            g[ab].layer = "roi_heads.mask.predictor.conv5_mask." + std::to_string(ab); g[ab].in = rows; g[ab].act = 1;
            g[ab].dst = (char*)up.d + (int64_t)(aa * 28 + bb) * 256 * (dt ? 2 : 4); g[ab].out_div = 14; g[ab].out_img_stride = (int64_t)2 * 28 * 256; g[ab].out_pix_stride = 2 * 256;
        }
        TRY(eng_conv_group(e, g));
    }
    const RawBuf *lw, *lb;
    void* p;
    TRY(need_tensor(e, "mask_logits.w", (int64_t)x.a.ncls * 256 * 4, &lw));
    TRY(need_tensor(e, "mask_logits.b", (int64_t)x.a.ncls * 4, &lb));
    TRY(eng_buf(e, "det.mask28", (int64_t)N * cap * 784 * 4, &p, 0, {N, cap, 28, 28}));
    {
        OpScope op(e, e.cur, "mask_logits_select (1x1 -> the label's channel + sigmoid)", (double)N * cap * 784 * (256.0 * (dt ? 2 : 4) + 4));
        if (dt) TRY(mask_logits_select_f16_launch(up.d, N * cap, 784, 256, (const float*)lw->d, (const float*)lb->d, x.a.d_out_labels, (float*)p, e.cur));
        else TRY(mask_logits_select_launch(up.d, N * cap, 784, 256, (const float*)lw->d, (const float*)lb->d, x.a.d_out_labels, (float*)p, e.cur));
    }
    eng_mark(e, "mask_head");
    return ISEGMI_OK;
}

static int maskrcnn_c4_forward(Engine& e, const float* d_images, int N);

// The FPN graph from the input to the box predictor's rows *cb, on the current canvas; leaves e.cur on the stream the RoI heads run on.  What the plain
// forward and the views of test-time augmentation (maskrcnn_aug_view) share.
static int fpn_to_predictor(RcnnCtx& x, const float* d_images, Tensor* cb) {
    Engine& e = x.e;
    if (e.cur_H % 32 || e.cur_W % 32) { set_error("Mask R-CNN input must be padded to a multiple of 32"); return ISEGMI_ERR_ARG; }
    e.cur = e.stream;
    eng_mark(e, "start");
    x.d_hw = (const int*)e.last_hw_ptr;  // maskrcnn_set_image_hw
    x.nms_flags = maskrcnn_nms_flags(e); x.roi_aligned = (int)e.param("roi_aligned", 0) ? 1 : 0;
    x.roi_table = (int)e.param("roi_table", x.dt ? 3.0f : 1.0f);
    rpn_config(x);
    TRY(rcnn_trunk(e, d_images, x.N, true, x.C));
    TRY(x.grp ? fpn_topdown_grouped(x) : fpn_topdown_levels(x));
    eng_mark(e, "fpn_topdown");
    TRY(fpn_out_and_rpn(x));
    eng_mark(e, "fpn_out+rpn");
    TRY(merge_proposals(x));
    eng_mark(e, "proposals");
    return box_head(x, cb);
}

int maskrcnn_forward(Engine& e, const float* d_images, int N) {
    TRY(keypoint_refusals(e));
    if (e.param("arch_c4", 0.0f) != 0.0f) return maskrcnn_c4_forward(e, d_images, N);
    RcnnCtx x{e, N, e.fp16 ? 1 : 0};
    Tensor cb;
    TRY(fpn_to_predictor(x, d_images, &cb));
    TRY(box_tail(e, N, x.fpn_post, cb, x.props, x.prop_cnt, x.d_hw, x.nms_flags, &x.a));
    eng_mark(e, "box_head");
    // Faster R-CNN (neither head): det.* is the result; the tail's bookkeeping as behind a head
    if (maskrcnn_keypoint_on(e)) TRY(keypoint_head(x));
    else if (maskrcnn_mask_on(e)) TRY(mask_head(x));
    TRY(eng_tail_end(e));
    e.cur = e.stream;
    return ISEGMI_OK;
}

// ---- test-time box augmentation: begin / view / merge
// What the augmented path is built for; everything else is refused by name.
static int aug_refusals(Engine& e) {
    const char* why = e.fp16 ? "fp16: test-time box augmentation is fp32 only"
                      : e.param("arch_c4", 0.0f) != 0.0f ? "arch_c4 (the R-50-C4 body): test-time box augmentation is built on the FPN bodies"
                      : e.param("graph", 0.0f) != 0.0f ? "graph 1: the views of test-time box augmentation change canvas and are not captured, set graph 0"
                      : maskrcnn_mask_on(e) ? "mask_on 1 (MODEL.MASK_ON True): test-time box augmentation returns boxes only, set mask_on 0"
                      : maskrcnn_keypoint_on(e) ? "keypoint_on 1 (MODEL.KEYPOINT_ON True): test-time box augmentation returns boxes only"
                      : nullptr;
    if (why) { set_error(std::string("bbox_aug (TEST.BBOX_AUG) with ") + why); return ISEGMI_ERR_STATE; }
    const int nc = (int)e.param("num_classes", 81.0f);
    if (nc < 2 || nc > 256) { set_error("bbox_aug (TEST.BBOX_AUG): num_classes (MODEL.ROI_BOX_HEAD.NUM_CLASSES) must be 2..256 (the merge sorts labels in one byte), got " + std::to_string(nc)); return ISEGMI_ERR_STATE; }
    const int R = (int)e.param("rpn_fpn_post_nms_top_n", 1000);   // before any view's forward is enqueued: the candidate stage holds 1024 rows per image
    if (R < 1 || R > 1024) { set_error("bbox_aug (TEST.BBOX_AUG): rpn_fpn_post_nms_top_n (MODEL.RPN.FPN_POST_NMS_TOP_N_TEST) must be 1..1024, got " + std::to_string(R)); return ISEGMI_ERR_STATE; }
    return ISEGMI_OK;
}

struct AugPool { float *boxes, *scores; int *labels, *cnt, *total; };
static int aug_pool(Engine& e, AugPool* p) {
    const int64_t N = e.max_batch, cap = e.aug_cap;
    void* q;
    TRY(eng_buf(e, "aug.pool_box", N * cap * 16, &q, 0, {N, cap, 4})); p->boxes = (float*)q;
    TRY(eng_buf(e, "aug.pool_score", N * cap * 4, &q, 0, {N, cap})); p->scores = (float*)q;
    TRY(eng_buf(e, "aug.pool_label", N * cap * 4, &q, 1, {N, cap})); p->labels = (int*)q;
    TRY(eng_buf(e, "aug.pool_cnt", N * 4, &q, 1, {N})); p->cnt = (int*)q;
    TRY(eng_buf(e, "aug.pool_total", N * 4, &q, 1, {N})); p->total = (int*)q;
    return ISEGMI_OK;
}

// The pool lives on the stream the RoI heads run on (the tail stream; the main stream without multi_stream): every launch that touches it goes there.
static hipStream_t aug_stream(Engine& e) { return e.multi_stream ? e.tail : e.stream; }

static int maskrcnn_aug_begin(Engine& e, int N, int pool_cap) {
    TRY(aug_refusals(e));
    ARG_CHECK(N > 0 && N <= e.max_batch, "batch size");
    if (pool_cap < 64 || pool_cap > 8192) { set_error("bbox_aug: pool_cap (BBoxAugConfig.POOL_CAP) must be 64..8192 (the merge sorts 8192 slots in LDS), got " + std::to_string(pool_cap)); return ISEGMI_ERR_ARG; }
    e.aug_N = N; e.aug_cap = pool_cap; e.aug_views = 0; e.aug_hw0.clear();
    AugPool p;
    TRY(aug_pool(e, &p));
    hipStream_t st = aug_stream(e);   // in stream order behind the previous sequence's merge and whatever read det.* there
    HIP_TRY(hipMemsetAsync(p.cnt, 0, (size_t)e.max_batch * 4, st));
    HIP_TRY(hipMemsetAsync(p.total, 0, (size_t)e.max_batch * 4, st));
    return ISEGMI_OK;
}

static int maskrcnn_aug_view(Engine& e, const float* d_images, const int32_t* h_image_hw, int N, int hflip, const float* h_ratios_wh) {
    TRY(aug_refusals(e));
    if (e.aug_N <= 0) { set_error("aug_view before aug_begin"); return ISEGMI_ERR_STATE; }
    ARG_CHECK(N == e.aug_N, "aug_view: the batch size aug_begin was given");
    if (e.aug_views == 0) e.aug_hw0.assign(h_image_hw, h_image_hw + 2 * N);
    RcnnCtx x{e, N, 0};
    Tensor cb;
    TRY(fpn_to_predictor(x, d_images, &cb));
    eng_mark(e, "box_head");
    BBoxAugArgs a;
    memset(&a, 0, sizeof(a));
    TRY(box_predictor_shape(e, cb.C, &a.ncls, &a.cls_agnostic));
    AugPool p;
    TRY(aug_pool(e, &p));
    void *rt, *ws;
    TRY(eng_buf(e, "aug.ratios", (int64_t)e.max_batch * 8, &rt));
    a.ws_bytes = bbox_aug_workspace_bytes(e.max_batch, 1024);
    TRY(eng_buf(e, "aug.ws", a.ws_bytes, &ws, 1));
    TRY(eng_stage_small(e, h_ratios_wh, (size_t)N * 8, rt, e.cur));   // behind the previous view's candidate stage, which read it on this stream
    a.N = N; a.R = x.fpn_post; a.hflip = hflip ? 1 : 0; a.cap = e.aug_cap;
    a.score_thresh = e.param("roi_score_thresh", 0.05f);
    a.logits_stride = cb.C; a.regr_stride = cb.C;
    a.d_logits = cb.d; a.d_regr = cb.d + a.ncls; a.d_props = x.props; a.d_prop_cnt = x.prop_cnt; a.d_image_hw = x.d_hw; a.d_ratios_wh = (const float*)rt;
    a.d_ws = ws;
    a.d_pool_boxes = p.boxes; a.d_pool_scores = p.scores; a.d_pool_labels = p.labels; a.d_pool_cnt = p.cnt; a.d_pool_total = p.total;
    {
        // logits + box regressions of every proposal once and the proposals in; at most the pool's slots out
        OpScope op(e, e.cur, "bbox_aug_candidates (softmax + decode + unflip + rescale, one view)", (double)N * a.R * ((double)cb.C * 4 + 16) + (double)N * e.aug_cap * 24);
        TRY(bbox_aug_candidates_launch(&a, e.cur));
    }
    eng_mark(e, "aug_candidates");
    ++e.aug_views;
    TRY(eng_tail_end(e));
    e.cur = e.stream;
    return ISEGMI_OK;
}

static int maskrcnn_aug_merge(Engine& e) {
    TRY(aug_refusals(e));
    if (e.aug_N <= 0 || e.aug_views <= 0) { set_error("aug_merge before aug_begin and at least one aug_view"); return ISEGMI_ERR_STATE; }
    const int N = e.aug_N, dpi = (int)e.param("detections_per_img", 100), cap = maskrcnn_det_cap(e);
    AugPool p;
    TRY(aug_pool(e, &p));
    isegmi_retina_post_args a;
    memset(&a, 0, sizeof(a));
    void* q;
    a.N = N; a.nseg = 1; a.seg_len = e.aug_cap; a.ncls = (int)e.param("num_classes", 81.0f); a.det_per_img = dpi; a.cap = cap;
    a.nms_flags = maskrcnn_nms_flags(e); a.nms_thresh = e.param("roi_nms_thresh", 0.5f);
    a.d_boxes = p.boxes; a.d_scores = p.scores; a.d_labels = p.labels; a.d_seg_cnt = p.cnt;
    a.ws_bytes = retina_post_workspace_bytes(e.max_batch, 1, e.aug_cap);
    TRY(eng_buf(e, "aug.merge_ws", a.ws_bytes, &q, 1)); a.d_ws = q;
    TRY(eng_buf(e, "det.count", (int64_t)N * 4, &q, 1, {N})); a.d_out_count = (int*)q;
    TRY(eng_buf(e, "det.box", (int64_t)N * cap * 16, &q, 0, {N, cap, 4})); a.d_out_boxes = (float*)q;
    TRY(eng_buf(e, "det.score", (int64_t)N * cap * 4, &q, 0, {N, cap})); a.d_out_scores = (float*)q;
    TRY(eng_buf(e, "det.label", (int64_t)N * cap * 4, &q, 1, {N, cap})); a.d_out_labels = (int*)q;
    hipStream_t st = aug_stream(e);
    {
        OpScope op(e, st, "bbox_aug_merge (class-wise NMS + detection cut over the pool)", (double)N * e.aug_cap * 24 + (double)N * cap * 24);
        TRY(retina_postprocess_launch(&a, st));
    }
    TRY(eng_tail_end(e));
    e.cur = e.stream;
    TRY(maskrcnn_set_image_hw(e, e.aug_hw0.data(), N));   // the sizes the results are in: view 0's
    e.last_N = N;
    e.aug_N = 0; e.aug_views = 0;
    return ISEGMI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// e2e_mask_rcnn_R_50_C4_1x (the config README.md:263-273 prints): ResNet-50 conv1..conv4 -> one stride-16 map (1024 ch) ->
// RPNHead (3x3 1024->1024, 15 anchors: 5 sizes x 3 ratios, ratio-major) -> top PRE_NMS_TOP_N_TEST (6000) -> decode / clip /
// NMS 0.7 -> POST_NMS_TOP_N_TEST (1000), no cross-level merge -> ROIAlign 14x14, 1/16, sampling_ratio 0 (adaptive) ->
// ResNet conv5 head (3 bottlenecks, the first with stride 2) -> 7x7x2048 -> AvgPool 7 -> FastRCNNPredictor (81 | 324) ->
// box post-processing as in the FPN model -> the SAME extractor on the detections (SHARE_BOX_FEATURE_EXTRACTOR) ->
// MaskRCNNC4Predictor: ConvTranspose 2x2/2 2048->256 + ReLU -> 1x1 -> 81 -> sigmoid, class-selected: 14x14 masks.
// fp32 only; single stream (the RoI heads are ~1.5 TFLOP per image here and dominate).
// (one set of weights, `prefix`, into the buffers of `tag`: the box and the mask branch each keep their own activations)
static int res5_head(Engine& e, const std::string& prefix, const std::string& tag, const Tensor& in, Tensor* out) {
    ResStage rs;
    rs.layers = prefix;
    rs.bufs = tag;
    rs.blocks = 3;
    rs.stride = 2;
    rs.stride_in_1x1 = true;
    return resnet_stage(e, rs, in, out);
}

static int maskrcnn_c4_forward(Engine& e, const float* d_images, int N) {
    const int H = e.cur_H, W = e.cur_W;
    const bool regen_anchors = e.capturing || e.anchor_H != H || e.anchor_W != W;
    if (H % 16 || W % 16) { set_error("Mask R-CNN C4 input must be padded to a multiple of 16"); return ISEGMI_ERR_ARG; }
    if (e.fp16) { set_error("the C4 configuration is fp32 only"); return ISEGMI_ERR_STATE; }
    if (e.multi_stream && e.tail_pending && !e.capturing) HIP_TRY(hipStreamWaitEvent(e.stream, e.tail_done, 0));
    e.cur = e.stream;
    hipStream_t st = e.stream;
    eng_mark(e, "start");
    void* p;
    const int* d_hw = (const int*)e.last_hw_ptr;  // maskrcnn_set_image_hw
    Tensor C[3];
    TRY(rcnn_trunk(e, d_images, N, false, C));
    Tensor C4 = C[2];  // [N, H/16, W/16, 1024]
    {   // expose under a stable name for tests
        Tensor alias;
        TRY(eng_act(e, "C4", N, C4.H, C4.W, C4.C, &alias));
        HIP_TRY(hipMemcpyAsync(alias.d, C4.d, (size_t)C4.numel() * 4, hipMemcpyDeviceToDevice, st));
        C4 = alias;
    }
    eng_mark(e, "backbone");

    // ---- RPN on the single map
    const int A = 15, CH = 75;
    const int pre_nms = (int)e.param("rpn_pre_nms_top_n", 6000), post_nms = (int)e.param("rpn_post_nms_top_n", 1000);
    const float rpn_thr = e.param("rpn_nms_thresh", 0.7f), rpn_min = e.param("rpn_min_size", 0.0f);
    const int ge = maskrcnn_nms_flags(e), roi_aligned = (int)e.param("roi_aligned", 0) ? 1 : 0;
    if (pre_nms > 6144 || post_nms > 1024) { set_error("C4 RPN: pre_nms <= 6144, post_nms <= 1024"); return ISEGMI_ERR_ARG; }
    Tensor t, head;
    TRY(eng_conv(e, "rpn.head.conv", C4, 1, 1, 1, nullptr, "rpn.t", &t));
    TRY(eng_conv(e, "rpn.head.cls_bbox", t, 1, 0, 0, nullptr, "rpn.head", &head));
    if (head.C != CH) { set_error("C4 rpn.head.cls_bbox must have 15 + 60 outputs"); return ISEGMI_ERR_STATE; }
    const int HWA = head.H * head.W * A;
    const float* anc; const RawBuf* base;
    TRY(need_tensor(e, "anchor_base.0", (int64_t)A * 16, &base));
    TRY(level_anchors(e, 0, *base, A, head.H, head.W, (int64_t)head.H * head.W, regen_anchors, &anc));
    e.anchor_H = H; e.anchor_W = W;
    const int R = post_nms;
    float *prob, *tkv, *props, *prop_scores; int *tki, *tkc, *prop_cnt;
    TRY(eng_buf(e, "rpn.prob", (int64_t)N * HWA * 4, &p)); prob = (float*)p;
    TRY(eng_buf(e, "rpn.tk_vals", (int64_t)N * pre_nms * 4, &p)); tkv = (float*)p;
    TRY(eng_buf(e, "rpn.tk_idx", (int64_t)N * pre_nms * 4, &p, 1)); tki = (int*)p;
    TRY(eng_buf(e, "rpn.tk_cnt", (int64_t)N * 4, &p, 1)); tkc = (int*)p;
    TRY(eng_buf(e, "proposals", (int64_t)N * R * 16, &p, 0, {N, R, 4})); props = (float*)p;
    TRY(eng_buf(e, "proposal_scores", (int64_t)N * R * 4, &p, 0, {N, R})); prop_scores = (float*)p;
    TRY(eng_buf(e, "proposal_count", (int64_t)N * 4, &p, 1, {N})); prop_cnt = (int*)p;
    TRY(rpn_sigmoid_launch(head.d, (int64_t)N * HWA, A, CH, prob, st));
    TRY(topk_launch(prob, HWA, N, HWA, pre_nms, nullptr, 1, tkv, tki, tkc, st));
    // one level: the NMS output (score order) IS the proposal list (select_over_all_levels only runs for > 1 level)
    void* nms_ws = nullptr;
    if (pre_nms <= 1024) TRY(eng_buf(e, "rpn.nms_ws", (int64_t)N * 131072, &nms_ws, 1));
    TRY(rpn_decode_nms_launch(head.d, anc, tkv, tki, tkc, d_hw, N, HWA, A, CH, pre_nms, post_nms, rpn_thr, rpn_min, ge, 0, 1,
                              R, props, prop_scores, prop_cnt, nms_ws, st));
    eng_mark(e, "rpn");

    // ---- box head: ROIAlign 14x14 (adaptive sampling) -> conv5 head -> avgpool -> predictors
    const float* feats[1] = {C4.d};
    const int Hs[1] = {C4.H}, Ws[1] = {C4.W};
    const float scales[1] = {0.0625f};
    Tensor roi, f5, pooled, cb;
    TRY(eng_act(e, "box.roi_feat", N * R, 14, 14, C4.C, &roi));
    TRY(roi_align_launch(feats, Hs, Ws, scales, 1, props, prop_cnt, N, R, C4.C, 14, 14, 0, 4, 0, roi.d, nullptr, st, nullptr, nullptr, roi_aligned));
    TRY(res5_head(e, "roi_heads.box.feature_extractor.head.layer4", "box.res5", roi, &f5));
    TRY(eng_act(e, "box.pooled", N * R, 1, 1, f5.C, &pooled));
    TRY(avgpool_full_launch(f5.d, (int64_t)N * R, f5.H * f5.W, f5.C, pooled.d, st));
    TRY(eng_conv(e, "roi_heads.box.predictor.cls_bbox", pooled, 1, 0, 0, nullptr, "box.cls_bbox", &cb));
    isegmi_box_post_args a;
    TRY(box_tail(e, N, R, cb, props, prop_cnt, d_hw, ge, &a));
    eng_mark(e, "box_head");
    if (!maskrcnn_mask_on(e)) {   // Faster R-CNN: no second pass of the conv5 head over the detections
        e.cur = e.stream;
        return ISEGMI_OK;
    }

    // ---- mask head: the shared extractor on the detections, then MaskRCNNC4Predictor
    const int cap = a.cap;
    Tensor mroi, m5, up;
    TRY(eng_act(e, "mask.roi_feat", N * cap, 14, 14, C4.C, &mroi));
    TRY(roi_align_launch(feats, Hs, Ws, scales, 1, a.d_out_boxes, a.d_out_count, N, cap, C4.C, 14, 14, 0, 4, 0, mroi.d, nullptr, st, nullptr, nullptr, roi_aligned));
    TRY(res5_head(e, "roi_heads.box.feature_extractor.head.layer4", "mask.res5", mroi, &m5));
    TRY(eng_act(e, "mask.deconv", N * cap, 14, 14, 256, &up));
    {
        Tensor rows;  // view: (roi, i) as "images" of 1 x 7 pixels
        rows.d = m5.d; rows.N = N * cap * 7; rows.H = 1; rows.W = 7; rows.C = m5.C; rows.dt = 0;
        for (int ab = 0; ab < 4; ++ab) {
            const int aa = ab >> 1, bb = ab & 1;
            TRY(eng_conv_into(e, "roi_heads.mask.predictor.conv5_mask." + std::to_string(ab), rows, 1, 0, 1,
                              (char*)up.d + (int64_t)(aa * 14 + bb) * 256 * 4, 7, (int64_t)2 * 14 * 256, 2 * 256));
        }
    }
    const RawBuf *lw, *lb;
    TRY(need_tensor(e, "mask_logits.w", (int64_t)a.ncls * 256 * 4, &lw));
    TRY(need_tensor(e, "mask_logits.b", (int64_t)a.ncls * 4, &lb));
    TRY(eng_buf(e, "det.mask14", (int64_t)N * cap * 196 * 4, &p, 0, {N, cap, 14, 14}));
    TRY(mask_logits_select_launch(up.d, N * cap, 196, 256, (const float*)lw->d, (const float*)lb->d, a.d_out_labels, (float*)p, st));
    eng_mark(e, "mask_head");
    e.cur = e.stream;
    return ISEGMI_OK;
}

// The per-image (w, h) resize ratios of the results stage in "ws.ratios", staged only when they changed: in stream order behind every earlier reader (the
// previous paste / box-record pack ran on a results stream this one is ordered behind).
int maskrcnn_stage_ratios(Engine& e, const float* h_ratios_wh, int N, hipStream_t ps, void** d_ratios) {
    void* rt;
    TRY(eng_buf(e, "ws.ratios", (int64_t)e.max_batch * 8, &rt));
    std::vector<float> now(h_ratios_wh, h_ratios_wh + 2 * N);
    if (now != e.last_ratios || e.last_ratios_ptr != (const void*)rt) {
        TRY(eng_stage_small(e, h_ratios_wh, (size_t)N * 8, rt, ps));
        e.last_ratios = now;
        e.last_ratios_ptr = rt;
    }
    *d_ratios = rt;
    return ISEGMI_OK;
}

int maskrcnn_paste(Engine& e, const float* h_ratios_wh, int out_h, int out_w) {
    const int N = e.last_N;
    if (N <= 0) { set_error("paste before forward"); return ISEGMI_ERR_STATE; }
    const int cap = maskrcnn_det_cap(e);
    if (!maskrcnn_mask_on(e)) { set_error("paste: the engine is box-only (mask_on 0, MODEL.MASK_ON False): there are no masks to paste"); return ISEGMI_ERR_STATE; }
    void *p, *rb, *rt;
    hipStream_t ps = eng_results_stream(e);
    e.cur = ps;
    TRY(maskrcnn_stage_ratios(e, h_ratios_wh, N, ps, &rt));
    TRY(eng_buf(e, "det.box_resized", (int64_t)N * cap * 16, &rb, 0, {N, cap, 4}));
    TRY(scale_boxes_launch((const float*)e.bufs["det.box"].d, (const float*)rt, N, cap, (float*)rb, ps));
    TRY(eng_buf(e, "det.masks", (int64_t)N * cap * out_h * out_w, &p, 2, {N, cap, out_h, out_w}));
    const bool c4 = e.param("arch_c4", 0.0f) != 0.0f;  // MaskRCNNC4Predictor emits 14x14 masks
    void* wq;
    TRY(eng_buf(e, "det.mask_window", (int64_t)e.max_batch * cap * 16, &wq, 1, {N, cap, 4}));
    // "sparse_masks": the planes are read through their windows only (isegmi_engine_rle: the device-side COCO output), so the 107 MB per image of
    // zero background need not be written; det.masks is then NOT a full binary plane (pixels outside a window are undefined)
    {
        // SURVEY 8d "Mask paste: read 0.31 MB, write <= 106 MB u8 per image": the planes are written whole unless sparse_masks (windows only: the
        // window bytes are data dependent and not counted here)
        const bool whole = e.param("sparse_masks", 0.0f) == 0.0f;
        OpScope op(e, ps, whole ? "paste_masks (Masker: resize + threshold + paste, whole uint8 planes)" : "paste_masks (sparse: box windows only)",
                   (double)N * cap * (c4 ? 196 : 784) * 4 + (whole ? (double)N * cap * out_h * out_w : 0.0));
        TRY(paste_masks_launch((const float*)e.bufs[c4 ? "det.mask14" : "det.mask28"].d, (const float*)rb, (const int*)e.bufs["det.count"].d, N,
                               cap, c4 ? 14 : 28, out_h, out_w, e.param("mask_threshold", 0.5f), (uint8_t*)p, ps, (int*)wq, whole));
    }
    if (ps == e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));
    e.cur = e.stream;
    eng_mark(e, "paste");
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_maskrcnn_forward_canvas(isegmi_engine* h, const float* d_images, const int32_t* h_image_hw, int N, int H, int W) {
    ARG_CHECK(h && d_images && h_image_hw, "null");
    ARG_CHECK(h->e.kind == 2, "engine is not a Mask R-CNN engine");
    Engine& e = h->e;
    TRY(rcnn_canvas_check(e, N, H, W));
    TRY(rcnn_begin_canvas(e, d_images, h_image_hw, N, H, W));
    char key[160];  // everything a captured graph bakes in: batch, canvas, input pointer, and which of the two image_hw buffers is current
    snprintf(key, sizeof(key), "maskrcnn:%d:%dx%d:%p:%p", N, H, W, (const void*)d_images, e.last_hw_ptr);
    const bool graph_on = e.param("graph", 0.0f) != 0.0f;
    const int rc = eng_graph_run(e, key, [&]() { return maskrcnn_forward(e, d_images, N); });
    if (graph_on) { e.anchor_H = -1; e.anchor_W = -1; }  // a replay leaves ITS canvas's anchors behind, whatever the bookkeeping says
    e.cur = e.stream;
    if (rc == ISEGMI_OK) e.last_N = N;
    return rc;
}

extern "C" int isegmi_maskrcnn_aug_begin(isegmi_engine* h, int N, int pool_cap) {
    ARG_CHECK(h, "null");
    ARG_CHECK(h->e.kind == 2, "engine is not a Mask R-CNN engine");
    return maskrcnn_aug_begin(h->e, N, pool_cap);
}

extern "C" int isegmi_maskrcnn_aug_view(isegmi_engine* h, const float* d_images, const int32_t* h_image_hw, int N, int H, int W, int hflip,
                                        const float* h_ratios_wh) {
    ARG_CHECK(h && d_images && h_image_hw && h_ratios_wh, "null");
    ARG_CHECK(h->e.kind == 2, "engine is not a Mask R-CNN engine");
    Engine& e = h->e;
    TRY(aug_refusals(e));
    TRY(rcnn_canvas_check(e, N, H, W));
    TRY(rcnn_begin_canvas(e, d_images, h_image_hw, N, H, W));
    const int rc = maskrcnn_aug_view(e, d_images, h_image_hw, N, hflip, h_ratios_wh);
    e.cur = e.stream;
    return rc;
}

extern "C" int isegmi_maskrcnn_aug_merge(isegmi_engine* h) {
    ARG_CHECK(h, "null");
    ARG_CHECK(h->e.kind == 2, "engine is not a Mask R-CNN engine");
    const int rc = maskrcnn_aug_merge(h->e);
    h->e.cur = h->e.stream;
    return rc;
}

extern "C" int isegmi_maskrcnn_forward(isegmi_engine* h, const float* d_images, const int32_t* h_image_hw, int N) {
    ARG_CHECK(h, "null");
    return isegmi_maskrcnn_forward_canvas(h, d_images, h_image_hw, N, h->e.H, h->e.W);
}

// h_ratios_wh [N][2] = (out_w / w_i, out_h / h_i) as float, computed by the host like BoxList.resize
extern "C" int isegmi_maskrcnn_paste(isegmi_engine* h, const float* h_ratios_wh, int out_h, int out_w) {
    ARG_CHECK(h && h_ratios_wh && out_h > 0 && out_w > 0, "paste args");
    ARG_CHECK(h->e.kind == 2, "engine is not a Mask R-CNN engine");
    return maskrcnn_paste(h->e, h_ratios_wh, out_h, out_w);
}

// One contiguous record block of the last Mask R-CNN forward for the all-gather:
//   [count i32 x N][box f32 x N*K*4][score f32 x N*K][label i32 x N*K][mask f32 x N*K*M*M]   (M = 28; 14 for the C4 predictor)
// (the 28x28 masks travel; the consumer pastes them).  D2D copies on the engine stream.
extern "C" int isegmi_maskrcnn_pack_records(isegmi_engine* h, void* d_dst, int64_t cap, int64_t* bytes) {
    ARG_CHECK(h && d_dst && bytes, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 2, "engine is not a Mask R-CNN engine");
    const int N = e.last_N;
    ARG_CHECK(N > 0, "pack before forward");
    ARG_CHECK(maskrcnn_mask_on(e), "pack_records carries the RoI masks: a box-only engine (mask_on 0) packs with isegmi_engine_pack_box_records");
    const int K = maskrcnn_det_cap(e);
    hipStream_t rs = eng_results_stream(e);
    const bool c4 = e.param("arch_c4", 0.0f) != 0.0f;  // MaskRCNNC4Predictor: 14x14 masks
    const int64_t msz = c4 ? 196 : 784;
    const char* names[5] = {"det.count", "det.box", "det.score", "det.label", c4 ? "det.mask14" : "det.mask28"};
    const int64_t sizes[5] = {(int64_t)N * 4, (int64_t)N * K * 16, (int64_t)N * K * 4, (int64_t)N * K * 4, (int64_t)N * K * msz * 4};
    int64_t off = 0;
    for (int i = 0; i < 5; ++i) {
        ARG_CHECK(off + sizes[i] <= cap, "record buffer too small");
        HIP_TRY(hipMemcpyAsync((char*)d_dst + off, e.bufs[names[i]].d, (size_t)sizes[i], hipMemcpyDeviceToDevice, rs));
        off += sizes[i];
    }
    if (rs == e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));
    *bytes = off;
    return ISEGMI_OK;
}
