// yolact.cpp -- the Yolact forward graph and its mask assembly.
//
// Yolact graph = SURVEY.md 8a Y2..Y7 (App. A.9): ResNet-50 (stride on the 3x3) -> FPN (bilinear
// top-down, relu'd 3x3 preds, two stride-2 downsamples) -> protonet on P3 -> shared prediction head
// on P3..P7 -> Detect -> postprocess.  BN is folded into the conv epilogue (scale, shift) by the
// Python host (isegmi/yolact.py) exactly once, in fp32.
#include <string.h>

#include "engine.h"

namespace isegmi {

// Points the engine's main / side streams and the names of the buffers eng_act allocates at lane e.lane for the duration of a forward.
struct LaneScope {
    Engine& e;
    explicit LaneScope(Engine& e_) : e(e_) { set(e.lane); if (e.lane) e.lane_tag = "@1"; }
    ~LaneScope() { set(0); e.lane_tag.clear(); e.cur = e.stream; }
    void set(int l) {
        if (e.lane_stream[l] == nullptr) return;
        e.stream = e.lane_stream[l];
        for (int k = 0; k < 3; ++k) e.side[k] = e.lane_side[l][k];
    }
};

// Redirects everything the rest of a forward launches (main stream, side streams, current stream) to the heads stream group.
struct HeadsScope {
    Engine& e;
    hipStream_t s, sd[3];
    bool on = false;
    explicit HeadsScope(Engine& e_) : e(e_), s(e_.stream) { for (int k = 0; k < 3; ++k) sd[k] = e.side[k]; }
    // wide = the group's branches (three laterals, protonet || prediction heads per level) on the group's own three side streams; otherwise they
    // queue on the heads stream one after the other (see yolact_forward)
    void enter(bool wide) { on = true; e.stream = e.heads; for (int k = 0; k < 3; ++k) e.side[k] = wide ? e.hside[k] : e.heads; e.cur = e.heads; }
    ~HeadsScope() { if (on) { e.stream = s; for (int k = 0; k < 3; ++k) e.side[k] = sd[k]; e.cur = s; } }
};

// ResNet-50 / -101, stride on the 3x3, a DCNv2 conv2 where the weights have one (YOLACT++) -> C[0..2] = res3.C, res4.C, res5.C
static int resnet_backbone(Engine& e, const float* d_images, int N, Tensor* C) {
    Tensor x;
    TRY(resnet_stem(e, "backbone.conv1", d_images, N, e.H, e.W, &x));
    eng_mark(e, "stem");
    const int blocks[4] = {3, 4, (int)e.param("resnet_depth", 50) == 101 ? 23 : 6, 3};
    for (int li = 0; li < 4; ++li) {
        ResStage s;
        s.layers = s.bufs = "backbone.layers." + std::to_string(li);
        s.blocks = blocks[li];
        s.stride = li > 0 ? 2 : 1;
        s.full = true;
        s.stage = "res" + std::to_string(li + 2);
        // C3 (then C4, C5) is about to be overwritten: the previous step's lateral convs, running on the heads streams, must have read them
        if (li == 1 && e.lat_pending[e.lane]) s.before_out = e.lat_done[e.lane];
        TRY(resnet_stage(e, s, x, &x));
        if (li >= 1) C[li - 1] = x;
        eng_mark(e, li == 0 ? "layer1" : li == 1 ? "layer2" : li == 2 ? "layer3" : "layer4");
    }
    return ISEGMI_OK;
}

// FPN: C[0..2] = C3, C4, C5 -> P[0..4] = P3..P7.  The three laterals are independent; so are the three prediction convs.  fp32 (round 5): each trio is
// ONE grouped launch (eng_conv_group), and so are the five levels' upfeature and head_cat convs of the heads: 16 launches become 4, and the small
// levels run inside the big level's launch instead of as 23-us launches of their own.  "conv_groups" 0 restores the per-layer launches (A/B; fp16 and
// the unfused head layout keep them anyway).
static int yolact_fpn(Engine& e, const Tensor* C, int N, bool grp, bool pipe, Tensor* P) {
    const int dt = e.fp16 ? 1 : 0;
    Tensor l5, l4, l3, x4f, x3f;
    if (grp) {
        std::vector<ConvGroupItem> g(3);
        g[0].layer = "fpn.lat_layers.2"; g[0].in = C[0]; g[0].out_name = "fpn.lat3"; g[0].out = &l3;
        g[1].layer = "fpn.lat_layers.1"; g[1].in = C[1]; g[1].out_name = "fpn.lat4"; g[1].out = &l4;
        g[2].layer = "fpn.lat_layers.0"; g[2].in = C[2]; g[2].out_name = "fpn.lat5"; g[2].out = &l5;
        TRY(eng_conv_group(e, g));
    } else {
        TRY(eng_fork(e, 0));
        TRY(eng_fork(e, 1));
        { SideScope sc(e, 0); TRY(eng_conv(e, "fpn.lat_layers.1", C[1], 1, 0, 0, nullptr, "fpn.lat4", &l4)); }
        { SideScope sc(e, 1); TRY(eng_conv(e, "fpn.lat_layers.2", C[0], 1, 0, 0, nullptr, "fpn.lat3", &l3)); }
        TRY(eng_conv(e, "fpn.lat_layers.0", C[2], 1, 0, 0, nullptr, "fpn.lat5", &l5));
        TRY(eng_join(e, 0));
        TRY(eng_join(e, 1));
    }
    if (pipe) { HIP_TRY(hipEventRecord(e.lat_done[e.lane], e.stream)); e.lat_pending[e.lane] = true; }
    TRY(eng_act(e, "fpn.x4", N, l4.H, l4.W, l4.C, &x4f, dt));
    if (dt) TRY(resize_bilinear_f16_launch(l5.d, N, l5.H, l5.W, l5.C, l4.H, l4.W, l4.d, 0, x4f.d, e.cur));
    else TRY(resize_bilinear_launch(l5.d, N, l5.H, l5.W, l5.C, l4.H, l4.W, l4.d, 0, x4f.d, e.cur));
    TRY(eng_act(e, "fpn.x3", N, l3.H, l3.W, l3.C, &x3f, dt));
    if (dt) TRY(resize_bilinear_f16_launch(x4f.d, N, x4f.H, x4f.W, x4f.C, l3.H, l3.W, l3.d, 0, x3f.d, e.cur));
    else TRY(resize_bilinear_launch(x4f.d, N, x4f.H, x4f.W, x4f.C, l3.H, l3.W, l3.d, 0, x3f.d, e.cur));
    if (grp) {
        std::vector<ConvGroupItem> g(3);
        g[0].layer = "fpn.pred_layers.2"; g[0].in = x3f; g[0].out_name = "P3"; g[0].out = &P[0];
        g[1].layer = "fpn.pred_layers.1"; g[1].in = x4f; g[1].out_name = "P4"; g[1].out = &P[1];
        g[2].layer = "fpn.pred_layers.0"; g[2].in = l5; g[2].out_name = "P5"; g[2].out = &P[2];
        for (auto& it : g) { it.pad = 1; it.act = 1; }
        TRY(eng_conv_group(e, g));
        TRY(eng_conv(e, "fpn.downsample_layers.0", P[2], 2, 1, 0, nullptr, "P6", &P[3]));
        TRY(eng_conv(e, "fpn.downsample_layers.1", P[3], 2, 1, 0, nullptr, "P7", &P[4]));
    } else {
        TRY(eng_fork(e, 0));
        TRY(eng_fork(e, 1));
        {
            SideScope sc(e, 0);  // P5 -> P6 -> P7 chain
            TRY(eng_conv(e, "fpn.pred_layers.0", l5, 1, 1, 1, nullptr, "P5", &P[2]));
            TRY(eng_conv(e, "fpn.downsample_layers.0", P[2], 2, 1, 0, nullptr, "P6", &P[3]));
            TRY(eng_conv(e, "fpn.downsample_layers.1", P[3], 2, 1, 0, nullptr, "P7", &P[4]));
        }
        { SideScope sc(e, 1); TRY(eng_conv(e, "fpn.pred_layers.1", x4f, 1, 1, 1, nullptr, "P4", &P[1])); }
        TRY(eng_conv(e, "fpn.pred_layers.2", x3f, 1, 1, 1, nullptr, "P3", &P[0]));
        TRY(eng_join(e, 0));
        TRY(eng_join(e, 1));
    }
    return ISEGMI_OK;
}

// What the shared prediction head leaves for Detect: either the fused rows (headcat) or the three separate tensors
struct HeadOut {
    int A = 0, Ptot = 0, CH = 0;
    bool fused = false;
    void *loc = nullptr, *conf = nullptr, *mask = nullptr, *headcat = nullptr;
    Tensor up[5];   // head.up0..4, the fused head's inputs (lazy_coeffs: the tail stream reads them again)
};
constexpr int kNumClasses = kYolactClasses, kMaskDim = kYolactMaskDim;

// ---- lazy_coeffs (fp32, fused head): the forward computes the loc|conf columns of the head only; see DESIGN.md section 4 "Mask coefficients of the kept
// detections only".
// Two views of the packed head_cat layer, built when the layer is registered: rows [0, 85 A) with their bias, and rows [85 A, 117 A) with theirs.  No copy:
// a view's pointers point into the layer's allocations.  A launch's weight descriptor spans the view's Cout rounded up to 128 rows (conv_fill's w_bytes),
// and a column tile reads whole tiles of rows: the first view's over-read rows are the layer's own next rows (their columns are past Cout and dropped), the
// second view's are the layer's zero padding rows -- provided 85 A + pad128(32 A) stays inside the layer's pad128(117 A) rows, which is checked here
// (A = 3: 255 + 128 <= 384; A = 9: 765 + 384 <= 1152).  Where it does not hold there are no views and the engine keeps the full head.
void yolact_head_views(Engine& e) {
    e.convs.erase(kHeadCatLocConf);
    e.convs.erase(kHeadCatCoeff);
    auto it = e.convs.find(kHeadCat);
    if (it == e.convs.end() || it->second.f16) return;
    const ConvLayer L = it->second;
    const int per = 4 + kNumClasses + kMaskDim;
    if (L.Cout % per != 0 || L.Cin % 32 != 0) return;
    const int A = L.Cout / per, split = A * (4 + kNumClasses);
    const int64_t wrow = (int64_t)L.R * L.S * L.Cin;
    auto packed_rows = [&](int cout) -> int64_t {
        isegmi_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.N = 1; d.H = L.R; d.W = L.S; d.Cin = L.Cin; d.Cout = cout; d.R = L.R; d.S = L.S; d.stride = 1;
        int64_t nf = 0;
        return isegmi_conv_packed_floats(&d, &nf) == ISEGMI_OK ? nf / wrow : -1;
    };
    const int64_t all = packed_rows(L.Cout), lo = packed_rows(split), hi = packed_rows(L.Cout - split);
    if (all < 0 || lo < 0 || hi < 0 || lo > all || split + hi > all) return;
    ConvLayer a = L, b = L;
    a.view = b.view = true;
    a.Cout = split;
    b.Cout = L.Cout - split;
    b.d_w = L.d_w + (int64_t)split * wrow;
    b.d_scale = L.d_scale ? L.d_scale + split : nullptr;
    b.d_shift = L.d_shift ? L.d_shift + split : nullptr;
    e.convs[kHeadCatLocConf] = a;
    e.convs[kHeadCatCoeff] = b;
}

// Does a forward of N images take the lazy schedule?  Parameter "lazy_coeffs": 1 on, 0 off (the schedule before it, launch for launch), -1 (default) by
// batch size: on from LAZY_COEFFS_MIN_BATCH images (profiles/lazy_coeffs.md).  fp16 and the unfused head keep the full head whatever it says.
constexpr int LAZY_COEFFS_MIN_BATCH = 3;
bool yolact_lazy_coeffs(Engine& e, int N) {
    if (e.kind != 1 || e.fp16 || e.convs.count(kHeadCatLocConf) == 0 || e.convs.count(kHeadCatCoeff) == 0) return false;
    const float p = e.param("lazy_coeffs", -1.0f);
    return p < 0.0f ? N >= LAZY_COEFFS_MIN_BATCH : p != 0.0f;
}

static void coeff_levels(const Tensor* up, CoeffLevels* lv) {
    lv->n = 5;
    for (int l = 0; l < 5; ++l) { lv->feat[l] = up[l].d; lv->H[l] = up[l].H; lv->W[l] = up[l].W; }
}

// A fetch of `headcat` after a lazy forward: run the coefficient view over all five levels into columns [85 A, 117 A) of the buffer, from the head.up<l>
// maps the forward left behind.  Everything the engine has in flight is waited for first and the fill itself is waited for, so no stream is left with
// new work or new dependencies; det.* and the pending-event flags are not touched.
int yolact_fill_coeff_columns(Engine& e) {
    const int N = e.last_N;
    auto hc = e.bufs.find("headcat");
    if (N <= 0 || hc == e.bufs.end() || e.convs.count(kHeadCatCoeff) == 0) { set_error("headcat: no lazy forward to complete"); return ISEGMI_ERR_STATE; }
    const int A = (int)e.param("num_priors", 3), CH = A * (4 + kNumClasses + kMaskDim);
    Tensor up[5];
    int64_t pix = 0, poff[5];
    for (int l = 0; l < 5; ++l) {
        auto it = e.bufs.find("head.up" + std::to_string(l));
        if (it == e.bufs.end() || it->second.shape.size() != 4 || it->second.shape[0] != N) { set_error("headcat: head.up maps missing"); return ISEGMI_ERR_STATE; }
        const RawBuf& b = it->second;
        up[l].d = (float*)b.d; up[l].N = N; up[l].H = (int)b.shape[1]; up[l].W = (int)b.shape[2]; up[l].C = (int)b.shape[3]; up[l].dt = 0;
        poff[l] = pix;
        pix += (int64_t)up[l].H * up[l].W;
    }
    if (hc->second.bytes < (int64_t)N * pix * CH * 4) { set_error("headcat: buffer smaller than the head.up maps imply"); return ISEGMI_ERR_STATE; }
    hipStream_t all[5] = {e.lane_stream[0], e.lane_stream[1], e.heads, e.tail, e.stream};
    for (hipStream_t st : all) if (st) HIP_TRY(hipStreamSynchronize(st));
    std::vector<ConvGroupItem> g(5);
    for (int l = 0; l < 5; ++l) {
        g[l].layer = kHeadCatCoeff; g[l].in = up[l]; g[l].pad = 1; g[l].act = 0;
        g[l].dst = (float*)hc->second.d + poff[l] * CH + A * (4 + kNumClasses); g[l].out_div = up[l].H * up[l].W;
        g[l].out_img_stride = pix * CH; g[l].out_pix_stride = CH; g[l].out_f32 = true;
    }
    // not a forward's launch: outside the conv timing / trace accounting
    const bool ct = e.conv_timing, tr = e.conv_trace;
    hipStream_t cur = e.cur;
    e.conv_timing = e.conv_trace = false;
    e.cur = e.stream;
    const int rc = eng_conv_group(e, g);
    e.conv_timing = ct; e.conv_trace = tr; e.cur = cur;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.coeff_cols_valid = true;
    return ISEGMI_OK;
}

// protonet on P3 and the shared prediction head on P3..P7
static int proto_and_heads(Engine& e, const Tensor* P, int N, bool grp, bool lazy, HeadOut* h) {
    const int dt = e.fp16 ? 1 : 0;
    // shared prediction head geometry
    const int A = (int)e.param("num_priors", 3), ncls = kNumClasses, md = kMaskDim;  // 9 for YOLACT++ (3 scales x 3 aspect ratios per cell)
    int Ptot = 0, off[5];
    for (int l = 0; l < 5; ++l) { off[l] = Ptot; Ptot += P[l].H * P[l].W * A; }
    {
        auto it = e.tensors.find("priors");
        if (it == e.tensors.end() || it->second.bytes != (int64_t)Ptot * 16) { set_error("priors tensor missing or wrong size"); return ISEGMI_ERR_STATE; }
    }
    // The three prediction convs (bbox 12, conf 243, mask 96) run as ONE 351-wide convolution when the host supplied
    // the fused layer: 6 instead of 1+4+2 64-wide column tiles per pixel tile, 5 launches instead of 15.  Its output
    // row per pixel is [A x 4 loc | A x 81 conf | A x 32 mask(pre-tanh)]; Detect reads it in place (HeadLayout).
    const bool fused = e.convs.count(kHeadCat) != 0;
    // lazy_coeffs: the loc|conf view of the layer (Cout = 85 A) into the same rows, same pixel stride CH; columns [85 A, CH) stay unwritten
    const char* head_layer = lazy ? kHeadCatLocConf : kHeadCat;
    const int CH = A * (4 + ncls + md);
    void *loc = nullptr, *conf = nullptr, *mask = nullptr, *headcat = nullptr;
    if (fused) {
        TRY(eng_buf(e, "headcat", (int64_t)N * (Ptot / A) * CH * 4, &headcat, 0, {N, Ptot / A, CH}));
    } else {
        TRY(eng_buf(e, "loc", (int64_t)N * Ptot * 4 * 4, &loc, 0, {N, Ptot, 4}));
        TRY(eng_buf(e, "conf", (int64_t)N * Ptot * ncls * 4, &conf, 0, {N, Ptot, ncls}));
        TRY(eng_buf(e, "mask", (int64_t)N * Ptot * md * 4, &mask, 0, {N, Ptot, md}));
    }
    Tensor* up = h->up;
    auto head_level = [&](int l) -> int {
        Tensor& uf = up[l];
        const std::string ln = "head.up" + std::to_string(l);
        TRY(eng_conv(e, "prediction_layers.0.upfeature.0", P[l], 1, 1, 1, nullptr, ln, &uf));
        const int hw = uf.H * uf.W;
        if (fused) {
            TRY(eng_conv_into(e, head_layer, uf, 1, 1, 0, (float*)headcat + (int64_t)(off[l] / A) * CH, hw,
                              (int64_t)(Ptot / A) * CH, CH, /*out_f32=*/true));
            return ISEGMI_OK;
        }
        TRY(eng_conv_into(e, "prediction_layers.0.bbox_layer", uf, 1, 1, 0, (float*)loc + (int64_t)off[l] * 4, hw, (int64_t)Ptot * 4, A * 4));
        TRY(eng_conv_into(e, "prediction_layers.0.conf_layer", uf, 1, 1, 0, (float*)conf + (int64_t)off[l] * ncls, hw, (int64_t)Ptot * ncls, A * ncls));
        TRY(eng_conv_into(e, "prediction_layers.0.mask_layer", uf, 1, 1, 2, (float*)mask + (int64_t)off[l] * md, hw, (int64_t)Ptot * md, A * md));
        return ISEGMI_OK;
    };
    // WAR: the previous forward's Detect / postprocess (tail stream) still reads loc/conf/mask/proto and the det.*
    // buffers; everything before this point touched only backbone/FPN buffers and was free to overlap with it.
    // (Two lanes: this wait is also what orders this step's heads phase behind the previous step's when pipeline_heads is off and the two
    // run on different lanes' main streams -- tail_done is recorded behind the previous step's Detect, which follows its heads.)
    if (e.multi_stream && e.tail_pending && !e.capturing) HIP_TRY(hipStreamWaitEvent(e.stream, e.tail_done, 0));
    // protonet (side 0) || heads on P3 (main) || heads on P4,P6 (side 1) || heads on P5,P7 (side 2)
    Tensor proto;
    TRY(eng_fork(e, 0));
    TRY(eng_fork(e, 1));
    TRY(eng_fork(e, 2));
    {
        SideScope sc(e, 0);
        Tensor t, u;
        TRY(eng_conv(e, "proto_net.0", P[0], 1, 1, 1, nullptr, "proto.t0", &t));
        TRY(eng_conv(e, "proto_net.2", t, 1, 1, 1, nullptr, "proto.t1", &u));
        TRY(eng_conv(e, "proto_net.4", u, 1, 1, 1, nullptr, "proto.t2", &t));
        TRY(eng_act(e, "proto.up", N, t.H * 2, t.W * 2, t.C, &u, dt));
        if (dt) TRY(resize_bilinear_f16_launch(t.d, N, t.H, t.W, t.C, t.H * 2, t.W * 2, nullptr, 1, u.d, e.cur));
        else TRY(resize_bilinear_launch(t.d, N, t.H, t.W, t.C, t.H * 2, t.W * 2, nullptr, 1, u.d, e.cur));
        TRY(eng_conv(e, "proto_net.8", u, 1, 1, 1, nullptr, "proto.t3", &t));
        TRY(eng_conv(e, "proto_net.10", t, 1, 0, 1, nullptr, "proto", &proto, /*out_f32=*/true));
    }
    if (grp) {   // the shared head over all five levels: upfeature x 5 as one launch, head_cat x 5 as one launch (main stream; the protonet on side 0)
        Tensor* uf = up;
        std::vector<ConvGroupItem> gu(5), gh(5);
        for (int l = 0; l < 5; ++l) {
            gu[l].layer = "prediction_layers.0.upfeature.0"; gu[l].in = P[l]; gu[l].pad = 1; gu[l].act = 1; gu[l].out_name = "head.up" + std::to_string(l); gu[l].out = &uf[l];
        }
        TRY(eng_conv_group(e, gu));
        for (int l = 0; l < 5; ++l) {
            gh[l].layer = head_layer; gh[l].in = uf[l]; gh[l].pad = 1; gh[l].act = 0;
            gh[l].dst = (float*)headcat + (int64_t)(off[l] / A) * CH; gh[l].out_div = uf[l].H * uf[l].W;
            gh[l].out_img_stride = (int64_t)(Ptot / A) * CH; gh[l].out_pix_stride = CH; gh[l].out_f32 = true;
        }
        TRY(eng_conv_group(e, gh));
    } else {
        { SideScope sc(e, 1); TRY(head_level(1)); TRY(head_level(3)); }
        { SideScope sc(e, 2); TRY(head_level(2)); TRY(head_level(4)); }
        TRY(head_level(0));
    }
    TRY(eng_join(e, 0));
    TRY(eng_join(e, 1));
    TRY(eng_join(e, 2));
    h->A = A; h->Ptot = Ptot; h->CH = CH; h->fused = fused;
    h->loc = loc; h->conf = conf; h->mask = mask; h->headcat = headcat;
    return ISEGMI_OK;
}

// Detect's argument block: parameters, the head's outputs, workspaces and the det.* result buffers
static int detect_args(Engine& e, int N, const HeadOut& h, isegmi_yolact_detect_args* out) {
    const int ncls = kNumClasses, md = kMaskDim, A = h.A, Ptot = h.Ptot;
    const int top_k = (int)e.param("nms_top_k", 200), max_det = (int)e.param("max_num_detections", 100);
    const int nc = ncls - 1;
    isegmi_yolact_detect_args& a = *out;
    memset(&a, 0, sizeof(a));
    a.N = N; a.P = Ptot; a.ncls = ncls; a.mask_dim = md; a.top_k = top_k; a.max_det = max_det;
    a.conf_thresh = e.param("nms_conf_thresh", 0.05f);
    a.nms_thresh = e.param("nms_thresh", 0.5f);
    a.second_threshold = (int)e.param("nms_second_threshold", 0) ? 1 : 0;   // App. A.6 fork (fast_nms(second_threshold=...)): default off
    // the suppression rule.  0 fast NMS (the default: nothing below changes), 1 cross-class fast NMS, 2 traditional per-class NMS
    const float fmode = e.param("nms_mode", 0.0f), fcap = e.param("nms_trad_cap", 1024.0f);
    if (fmode != 0.0f && fmode != 1.0f && fmode != 2.0f) { set_error("nms_mode must be 0 (fast), 1 (cross-class fast) or 2 (traditional)"); return ISEGMI_ERR_ARG; }
    const int mode = (int)fmode, cap = (int)fcap;
    if ((float)cap != fcap || cap < 64 || cap > 2048 || cap % 64 != 0) { set_error("nms_trad_cap must be a multiple of 64 in [64, 2048]"); return ISEGMI_ERR_ARG; }
    if (mode != 0 && a.second_threshold) { set_error("nms_second_threshold is an argument of fast_nms only: not with nms_mode 1 or 2"); return ISEGMI_ERR_ARG; }
    a.nms_mode = mode; a.trad_cap = cap; a.trad_scale = e.param("max_size", 550.0f);
    const int tkw = mode == 2 ? cap : top_k;   // width of the per-class sorted rows
    if (h.fused) {
        a.d_conf = a.d_loc = a.d_mask = (const float*)h.headcat;
        a.A = A; a.pix_stride = h.CH; a.off_loc = 0; a.off_conf = A * 4; a.off_mask = A * 4 + A * ncls; a.mask_tanh = 1;
    } else {
        a.d_conf = (const float*)h.conf; a.d_loc = (const float*)h.loc; a.d_mask = (const float*)h.mask;
    }
    a.d_priors = (const float*)e.tensors["priors"].d;
    void* p;
    TRY(eng_buf(e, "ws.scoresT", (int64_t)N * nc * Ptot * 4, &p)); a.d_ws_scoresT = (float*)p;
    TRY(eng_buf(e, "boxes_all", (int64_t)N * Ptot * 16, &p, 0, {N, Ptot, 4})); a.d_ws_boxes = (float*)p;
    TRY(eng_buf(e, "ws.counts", (int64_t)2 * N * 4, &p, 1)); a.d_ws_counts = (int32_t*)p;
    TRY(eng_buf(e, "ws.tk_vals", (int64_t)N * nc * tkw * 4, &p)); a.d_ws_tk_vals = (float*)p;
    TRY(eng_buf(e, "ws.tk_idx", (int64_t)N * nc * tkw * 4, &p, 1)); a.d_ws_tk_idx = (int32_t*)p;
    TRY(eng_buf(e, "ws.tk_cnt", (int64_t)N * nc * 4, &p, 1)); a.d_ws_tk_cnt = (int32_t*)p;
    TRY(eng_buf(e, "ws.cand", (int64_t)N * nc * (mode == 2 ? 128 : top_k) * 4, &p)); a.d_ws_cand = (float*)p;
    if (mode != 0) {   // the default mode allocates and launches exactly what it did before the modes existed
        TRY(eng_buf(e, "det.nms_total", (int64_t)N * 4, &p, 1, {N})); a.d_out_nms_total = (int32_t*)p;
        TRY(eng_buf(e, "det.nms_overflow", (int64_t)N * 4, &p, 1, {N})); a.d_out_nms_overflow = (int32_t*)p;
    }
    if (mode == 1) {
        TRY(eng_buf(e, "ws.cc_scores", (int64_t)N * Ptot * 4, &p)); a.d_ws_cc_scores = (float*)p;
        TRY(eng_buf(e, "ws.cc_class", (int64_t)N * Ptot * 4, &p, 1)); a.d_ws_cc_class = (int32_t*)p;
    }
    if (mode == 2) {
        TRY(eng_buf(e, "ws.trad_list", (int64_t)(1 + N * nc) * 4, &p, 1)); a.d_ws_trad_list = (int32_t*)p;
        TRY(eng_buf(e, "ws.trad_prior", (int64_t)N * nc * 128 * 4, &p, 1)); a.d_ws_trad_prior = (int32_t*)p;
    }
    TRY(eng_buf(e, "ws.fin_vals", (int64_t)N * max_det * 4, &p)); a.d_ws_fin_vals = (float*)p;
    TRY(eng_buf(e, "ws.fin_idx", (int64_t)N * max_det * 4, &p, 1)); a.d_ws_fin_idx = (int32_t*)p;
    TRY(eng_buf(e, "ws.fin_cnt", (int64_t)N * 4, &p, 1)); a.d_ws_fin_cnt = (int32_t*)p;
    TRY(eng_buf(e, "det.count", (int64_t)N * 4, &p, 1, {N})); a.d_out_count = (int32_t*)p;
    TRY(eng_buf(e, "det.box", (int64_t)N * max_det * 16, &p, 0, {N, max_det, 4})); a.d_out_boxes = (float*)p;
    TRY(eng_buf(e, "det.score", (int64_t)N * max_det * 4, &p, 0, {N, max_det})); a.d_out_scores = (float*)p;
    TRY(eng_buf(e, "det.class", (int64_t)N * max_det * 4, &p, 1, {N, max_det})); a.d_out_classes = (int32_t*)p;
    TRY(eng_buf(e, "det.coeff", (int64_t)N * max_det * md * 4, &p, 0, {N, max_det, md})); a.d_out_coeffs = (float*)p;
    TRY(eng_buf(e, "det.prior", (int64_t)N * max_det * 4, &p, 1, {N, max_det})); a.d_out_prior = (int32_t*)p;
    return ISEGMI_OK;
}

int yolact_forward(Engine& e, const float* d_images, int N) {
    LaneScope lscope(e);
    e.cur = e.stream;
    // cross-step pipelining of the heads phase (eager multi-stream throughput mode only)
    const bool pipe = e.multi_stream && !e.capturing && !e.timing && !e.conv_timing && e.heads != nullptr &&
                      e.param("graph", 0.0f) == 0.0f && e.param("pipeline_heads", 1.0f) != 0.0f;
    HeadsScope hscope(e);
    eng_mark(e, "start");
    const int dt = e.fp16 ? 1 : 0;  // fp16 storage + f16 MFMA convolutions (optional mode; heads / prototypes / Detect stay fp32)
    if (dt && e.convs.count("prediction_layers.0.head_cat") == 0) { set_error("fp16 Yolact needs the fused prediction head"); return ISEGMI_ERR_STATE; }
    Tensor C[3], P[5];   // C3-C5, P3-P7
    // yolact_darknet53_config.  C3 (then C4, C5) is about to be overwritten there: the previous step's lateral convs must have read them
    if (e.param("darknet", 0.0f) != 0.0f) TRY(darknet_backbone(e, "backbone.", d_images, N, C, e.lat_pending[e.lane] ? e.lat_done[e.lane] : nullptr));
    else TRY(resnet_backbone(e, d_images, N, C));
    if (pipe) {  // hand the rest of this forward to the heads stream group; the caller's next forward starts its backbone at once
        hipEvent_t ev;
        TRY(eng_next_event(e, &ev));
        HIP_TRY(hipEventRecord(ev, e.stream));
        HIP_TRY(hipStreamWaitEvent(e.heads, ev, 0));
        // Side streams for the heads group only where a forward is latency-bound (small batches: bs=1 p50 1.98 vs 2.24 ms).  At the bench batch two
        // concurrent streams of chip-filling convolutions (backbone i+1 || heads i) leave nothing for more streams to fill, and every extra stream
        // is one more for the runtime to fold onto its four in-order hardware queues, where a branch then waits behind kernels of the other group
        // it does not depend on: without them +1-4 % (Yolact fp32 / yolact_base / fp16 bs=8; profiles/r03_experiments.txt 3c).  Parameter
        // "heads_side_streams": 1 always, 0 never, default by batch size.
        const float hs = e.param("heads_side_streams", -1.0f);
        hscope.enter(hs < 0.0f ? N <= 2 : hs != 0.0f);
    } else if (e.heads_pending) {  // mode switch without a sync in between: an earlier pipelined heads phase writes the same buffers
        HIP_TRY(hipStreamWaitEvent(e.stream, e.heads_done, 0));
        e.heads_pending = false;
    }
    const bool grp = !dt && e.param("conv_groups", 1.0f) != 0.0f && e.param("conv_tile", 0) == 0.0f && e.convs.count(kHeadCat) != 0;
    const bool lazy = yolact_lazy_coeffs(e, N);
    if (!lazy && !dt && e.param("lazy_coeffs", -1.0f) > 0.0f && e.convs.count(kHeadCat) != 0) {
        set_error("lazy_coeffs: the fused head's rows do not split inside its padded weight image");
        return ISEGMI_ERR_STATE;
    }
    TRY(yolact_fpn(e, C, N, grp, pipe, P));
    eng_mark(e, "fpn");
    e.lane_tag.clear();   // everything allocated from here on (protonet, heads, Detect) exists once: it runs in step order behind the WAR point in proto_and_heads
    HeadOut head;
    TRY(proto_and_heads(e, P, N, grp, lazy, &head));
    eng_mark(e, "proto+heads");
    isegmi_yolact_detect_args a;
    TRY(detect_args(e, N, head, &a));
    // Detect is a chain of small latency-bound grids: run it (and postprocess) on the tail stream so the NEXT
    // forward's MFMA-bound backbone can start underneath it.
    hipStream_t ds = e.stream;
    if (e.multi_stream) {
        hipEvent_t ev;
        TRY(eng_next_event(e, &ev));
        HIP_TRY(hipEventRecord(ev, e.stream));
        HIP_TRY(hipStreamWaitEvent(e.tail, ev, 0));
        ds = e.tail;
    }
    {
        // confidences and box regressions of every prior once (the fused head's [N][P][4 + 81] columns) + priors + the mask coefficients of
        // the kept detections (the gather reads no other prior's)
        OpScope op(e, ds, "yolact_detect (softmax + decode + per-class top-k + fast-NMS + gather)",
                   (double)N * a.P * ((double)(4 + a.ncls - 1) * 4) + (double)a.P * 16 + (double)N * a.max_det * a.mask_dim * 4);
        if (lazy) {
            // Detect split at the final top-k: the kept slots' rows, their 32 coefficients each from head.up<level> (ordered behind the heads phase by the
            // event above; the next forward's writers of head.up wait on tail_done), then the gather from ws.coeff_sel
            const ConvLayer& Lc = e.convs[kHeadCatCoeff];
            CoeffLevels lv;
            coeff_levels(head.up, &lv);
            void *rows, *sel;
            TRY(eng_buf(e, "ws.coeff_rows", (int64_t)N * a.max_det * 5 * 4, &rows, 1));
            TRY(eng_buf(e, "ws.coeff_sel", (int64_t)N * a.max_det * a.mask_dim * 4, &sel, 0, {N, a.max_det, a.mask_dim}));
            TRY(yolact_detect_select_launch(&a, ds));
            const int32_t* sel_idx; int sel_nc, sel_k;   // where the final top-k's flat indices point in this nms_mode
            yolact_detect_index_view(&a, &sel_idx, &sel_nc, &sel_k);
            TRY(yolact_coeff_index_launch(a.d_ws_fin_idx, sel_idx, a.d_ws_fin_cnt, N, sel_nc, sel_k, a.max_det, head.A, lv, (int32_t*)rows, ds));
            TRY(yolact_coeff_rows_launch(lv, N, Lc.Cin, Lc.R, Lc.S, 1, Lc.d_w, Lc.d_scale, Lc.d_shift, head.A, 0, a.mask_dim, (const int32_t*)rows,
                                         a.d_ws_fin_cnt, a.max_det, (float*)sel, ds));
            TRY(yolact_detect_gather_launch(&a, (const float*)sel, ds));
        } else {
            TRY(yolact_detect_launch(&a, ds));
        }
    }
    if (pipe) { HIP_TRY(hipEventRecord(e.heads_done, e.stream)); e.heads_pending = true; }
    TRY(eng_tail_end(e));
    eng_mark(e, "detect");
    return ISEGMI_OK;
}

// h_image_hw (optional, [N][2]): image n is assembled at its own (h_n, w_n) inside the common (h, w) plane
int yolact_postprocess(Engine& e, int h, int w, const int32_t* h_image_hw) {
    const int N = e.last_N;
    if (N <= 0) { set_error("postprocess before forward"); return ISEGMI_ERR_STATE; }
    const int K = (int)e.param("max_num_detections", 100);
    RawBuf& proto = e.bufs["proto"];
    const int PH = (int)proto.shape[1], PW = (int)proto.shape[2], md = (int)proto.shape[3];
    void *lo, *masks, *ib;
    hipStream_t rs = eng_results_stream(e);
    int* d_ihw = nullptr;
    if (h_image_hw) {
        for (int i = 0; i < N; ++i)
            if (h_image_hw[2 * i] <= 0 || h_image_hw[2 * i] > h || h_image_hw[2 * i + 1] <= 0 || h_image_hw[2 * i + 1] > w) { set_error("postprocess: image size outside the plane"); return ISEGMI_ERR_ARG; }
        void* q;
        TRY(eng_buf(e, "pp.image_hw", (int64_t)e.max_batch * 8, &q, 1, {N, 2}));
        d_ihw = (int*)q;
        TRY(eng_stage_small(e, h_image_hw, (size_t)N * 8, d_ihw, rs));
    }
    TRY(eng_buf(e, "ws.lo", (int64_t)N * K * PH * PW * 4, &lo));
    TRY(eng_buf(e, "det.masks", (int64_t)N * K * h * w, &masks, 2, {N, K, h, w}));
    TRY(eng_buf(e, "det.box_int", (int64_t)N * K * 4 * 8, &ib, 3, {N, K, 4}));
    void* wq;
    TRY(eng_buf(e, "det.mask_window", (int64_t)e.max_batch * K * 16, &wq, 1, {N, K, 4}));
    {
        // SURVEY 8d "Yolact assembly: read the prototypes + coefficients, write n x h x w" (uint8 planes; whole unless sparse_masks)
        const bool whole = e.param("sparse_masks", 0.0f) == 0.0f;
        OpScope op(e, rs, whole ? "yolact_masks (proto @ coeff -> sigmoid -> crop -> upsample -> threshold, whole uint8 planes)" : "yolact_masks (sparse: box windows only)",
                   (double)N * PH * PW * md * 4 + (double)N * K * md * 4 + (whole ? (double)N * K * h * w : 0.0));
        TRY(yolact_masks_launch((const float*)proto.d, (const float*)e.bufs["det.coeff"].d, (const float*)e.bufs["det.box"].d,
                                (const int*)e.bufs["det.count"].d, N, PH, PW, md, K, h, w, (float*)lo, (uint8_t*)masks, (int64_t*)ib,
                                rs, d_ihw, (int*)wq, whole, /*dense_lo=*/e.convs.count("maskiou_net.2") != 0));
    }
    if (e.convs.count("maskiou_net.2")) {
        // YOLACT++ fast mask re-scoring on the proto-resolution masks just written to ws.lo: first layer (1 input channel) and
        // the global-max / class pick as small dedicated kernels, the rest on the MFMA conv kernels over all N*K slots
        auto w0 = e.tensors.find("maskiou.w0"), b0 = e.tensors.find("maskiou.b0");
        if (w0 == e.tensors.end() || b0 == e.tensors.end()) { set_error("maskiou_net.0 weights missing"); return ISEGMI_ERR_STATE; }
        hipStream_t saved = e.cur;
        e.cur = rs;
        Tensor t, u;
        TRY(eng_act(e, "maskiou.t0", N * K, (PH - 3) / 2 + 1, (PW - 3) / 2 + 1, 32, &t));
        TRY(maskiou_conv1_launch((const float*)lo, N * K, PH, PW, (const float*)w0->second.d, (const float*)b0->second.d, t.d, rs));
        for (int i = 2; i <= 8; i += 2) {
            if (t.H < 3 || t.W < 3) { e.cur = saved; set_error("input too small for the mask-IoU net (five stride-2 3x3 convs)"); return ISEGMI_ERR_ARG; }
            TRY(eng_conv(e, "maskiou_net." + std::to_string(i), t, 2, 0, 1, nullptr, "maskiou.t" + std::to_string(i), &u));
            t = u;
        }
        TRY(eng_conv(e, "maskiou_net.10", t, 1, 0, 1, nullptr, "maskiou.cls", &u));
        void* ms;
        TRY(eng_buf(e, "det.mask_score", (int64_t)N * K * 4, &ms, 0, {N, K}));
        TRY(maskiou_rescore_launch(u.d, N, K, u.H * u.W, u.C, (const int*)e.bufs["det.class"].d, (const float*)e.bufs["det.score"].d,
                                   (const int*)e.bufs["det.count"].d, (float*)ms, rs));
        e.cur = saved;
    }
    if (rs == e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));
    eng_mark(e, "masks");
    return ISEGMI_OK;
}

}  // namespace isegmi
