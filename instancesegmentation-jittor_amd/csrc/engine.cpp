// engine.cpp -- engine object behind the C ABI: weights, buffers, conv launches, streams and lanes, uploads, timings.  The models' forward graphs
// are in yolact.cpp, maskrcnn.cpp, pose2seg.cpp, retinanet.cpp and yolov3.cpp, over the trunks of resnet.cpp and darknet.cpp.
#include <mutex>
#include "engine.h"

#include <string.h>

namespace isegmi {

int eng_buf(Engine& e, const std::string& name, int64_t bytes, void** out, int dtype, std::vector<int64_t> shape) {
    RawBuf& b = e.bufs[name];
    if (b.bytes < bytes) {
        if (e.capturing) { set_error("buffer " + name + " would be (re)allocated during graph capture"); return ISEGMI_ERR_STATE; }
        // a captured graph holds the old device pointers of every buffer it touches: a grown buffer (a larger canvas or batch after a smaller one;
        // the liveness-aliased res<l>.* buffers are shared by many layers) invalidates all of them -- they are re-captured on their next use
        if (b.d) {
            HIP_TRY(hipFree(b.d));  // (synchronises the device: no replay is in flight when the graphs go)
            if (!e.graphs.empty()) eng_graph_reset(e);
        }
        b.d = nullptr;
        HIP_TRY(hipMalloc(&b.d, (size_t)(bytes > 0 ? bytes : 16)));
        b.bytes = bytes;
    }
    b.dtype = dtype;
    b.shape = shape;
    *out = b.d;
    return ISEGMI_OK;
}

int eng_act(Engine& e, const std::string& name, int N, int H, int W, int C, Tensor* t, int dt) {
    void* p = nullptr;
    int rc = eng_buf(e, e.lane_tag.empty() ? name : name + e.lane_tag, (int64_t)N * H * W * C * (dt ? 2 : 4), &p, dt ? 4 : 0, {N, H, W, C});
    if (rc) return rc;
    t->d = (float*)p; t->N = N; t->H = H; t->W = W; t->C = C; t->dt = dt;
    return ISEGMI_OK;
}

static int find_conv(Engine& e, const std::string& layer, const ConvLayer** out) {
    auto it = e.convs.find(layer);
    if (it == e.convs.end()) { set_error("conv layer not set: " + layer); return ISEGMI_ERR_STATE; }
    *out = &it->second;
    return ISEGMI_OK;
}

static int timed_conv(Engine& e, const std::string& label, const isegmi_conv_desc* d, const float* in, const ConvLayer* L, const float* res, void* out,
                      bool out_f32 = false) {
    const int Ho = (d->H + 2 * d->pad - d->R) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->S) / d->stride + 1;
    ConvScope cs(e);
    cs.trace(label, "", d->N, d->H, d->W, d->Cin, d->Cout, d->R, d->stride, Ho * Wo * d->N, res != nullptr);
    if (L->groups > 1) {   // a grouped layer does Cin / groups products per output: its algorithmic FLOPs are the dense ones over `groups`
        TRY(conv2d_grouped_launch(d, L->groups, in, L->d_w, L->d_scale, L->d_shift, res, (float*)out, e.cur));
        cs.done(2.0 * d->N * Ho * Wo * (double)d->Cout * d->R * d->S * (d->Cin / L->groups), "%s [M=%d K=%d Cout=%d %dx%d/%d groups=%d]", label.c_str(),
                d->N * Ho * Wo, d->R * d->S * (d->Cin / L->groups), d->Cout, d->R, d->S, d->stride, L->groups);
        return ISEGMI_OK;
    }
    TRY(L->f16 ? conv2d_f16_launch(d, in, L->d_w, L->d_scale, L->d_shift, res, out, out_f32 ? 1 : 0, e.cur)
               : conv2d_launch(d, in, L->d_w, L->d_scale, L->d_shift, res, (float*)out, e.cur));
    const int cin_true = (d->Cin == 4 && d->R == 7) ? 3 : d->Cin;   // the stem's fourth input channel is padding
    cs.done(2.0 * d->N * Ho * Wo * (double)d->Cout * d->R * d->S * cin_true, "%s [M=%d K=%d Cout=%d %dx%d/%d]", label.c_str(), d->N * Ho * Wo,
            d->R * d->S * d->Cin, d->Cout, d->R, d->S, d->stride);
    return ISEGMI_OK;
}

int eng_conv_into(Engine& e, const std::string& layer, const Tensor& in, int stride, int pad, int act, void* dst, int out_div,
                  int64_t out_img_stride, int64_t out_pix_stride, bool out_f32, const float* residual) {
    const ConvLayer* L;
    int rc = find_conv(e, layer, &L);
    if (rc) return rc;
    if (L->Cin != in.C) { set_error("conv " + layer + ": Cin mismatch"); return ISEGMI_ERR_ARG; }
    if ((in.dt == 1) != L->f16) { set_error("conv " + layer + ": activation / weight precision mismatch"); return ISEGMI_ERR_STATE; }
    if (L->groups > 1) { set_error("conv " + layer + ": a grouped layer writes a dense output only"); return ISEGMI_ERR_ARG; }
    if (residual && L->f16) { set_error("conv " + layer + ": a strided destination takes an fp32 residual only"); return ISEGMI_ERR_ARG; }
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = in.N; d.H = in.H; d.W = in.W; d.Cin = in.C; d.Cout = L->Cout; d.R = L->R; d.S = L->S; d.stride = stride; d.pad = pad;
    d.act = act; d.tile = (int)e.param("conv_tile", 0); d.out_div = out_div; d.out_img_stride = out_img_stride;
    d.out_pix_stride = out_pix_stride;
    return timed_conv(e, layer, &d, in.d, L, residual, dst, out_f32);
}

int eng_conv(Engine& e, const std::string& layer, const Tensor& in, int stride, int pad, int act, const Tensor* residual,
             const std::string& out_name, Tensor* out, bool out_f32, bool may_split) {
    const ConvLayer* L;
    int rc = find_conv(e, layer, &L);
    if (rc) return rc;
    if (L->Cin != in.C) { set_error("conv " + layer + ": Cin mismatch"); return ISEGMI_ERR_ARG; }
    if ((in.dt == 1) != L->f16) { set_error("conv " + layer + ": activation / weight precision mismatch"); return ISEGMI_ERR_STATE; }
    if (residual && residual->dt != in.dt) { set_error("conv " + layer + ": residual precision mismatch"); return ISEGMI_ERR_STATE; }
    const int Ho = (in.H + 2 * pad - L->R) / stride + 1, Wo = (in.W + 2 * pad - L->S) / stride + 1;
    rc = eng_act(e, out_name, in.N, Ho, Wo, L->Cout, out, (L->f16 && !out_f32) ? 1 : 0);
    if (rc) return rc;
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = in.N; d.H = in.H; d.W = in.W; d.Cin = in.C; d.Cout = L->Cout; d.R = L->R; d.S = L->S; d.stride = stride; d.pad = pad;
    d.act = act; d.tile = (int)e.param("conv_tile", 0);
    // `conv_split_k` (default 0): the fixed-tree split-K evaluation (conv tile 15) for the backbone's bottleneck convolutions the caller
    // marks -- every conv2 / conv3 and the conv1 of a stage's later blocks -- where the shape rule takes them (small M, K >= 1024: a bs = 1 forward).  An
    // OPT-IN NUMERICS MODE: results are bit-exact against the oracle models run with conv_split_k (the same layers, the same rule), not against the default.
    if (may_split && !L->f16 && L->groups == 1 && d.tile == 0 && (int)e.param("conv_split_k", 0) != 0 && isegmi_conv_split_qualifies(&d)) d.tile = 15;
    if (L->groups > 1) d.tile = 0;   // one kernel, one k-ordered chain per output: never split-K whatever the shape rule says, no forced tile
    return timed_conv(e, layer, &d, in.d, L, residual ? residual->d : nullptr, out->d, out_f32);
}

int eng_conv_group(Engine& e, std::vector<ConvGroupItem>& items) {
    const int n = (int)items.size();
    if (n == 0) return ISEGMI_OK;
    bool grouped = n > 1 && n <= 10 && e.param("conv_groups", 1.0f) != 0.0f && e.param("conv_tile", 0) == 0.0f;
    std::vector<const ConvLayer*> Ls(n);
    for (int i = 0; i < n; ++i) {
        int rc = find_conv(e, items[i].layer, &Ls[i]);
        if (rc) return rc;
        if (Ls[i]->f16 || items[i].in.dt == 1 || (Ls[i]->Cin == 4 && Ls[i]->R == 7) || Ls[i]->groups > 1) grouped = false;
    }
    if (!grouped) {
        for (auto& it : items) {
            int rc = it.dst ? eng_conv_into(e, it.layer, it.in, it.stride, it.pad, it.act, it.dst, it.out_div, it.out_img_stride, it.out_pix_stride, it.out_f32)
                            : eng_conv(e, it.layer, it.in, it.stride, it.pad, it.act, it.residual, it.out_name, it.out, it.out_f32);
            if (rc) return rc;
        }
        return ISEGMI_OK;
    }
    std::vector<isegmi_conv_desc> ds(n);
    std::vector<const isegmi_conv_desc*> dp(n);
    std::vector<const float*> in(n), w(n), sc(n), sh(n), rs(n);
    std::vector<float*> out(n);
    std::vector<int> M(n);
    double fl = 0;
    std::string label = "group[";
    for (int i = 0; i < n; ++i) {
        ConvGroupItem& it = items[i];
        const ConvLayer* L = Ls[i];
        if (L->Cin != it.in.C) { set_error("conv " + it.layer + ": Cin mismatch"); return ISEGMI_ERR_ARG; }
        if (it.residual && it.residual->dt != it.in.dt) { set_error("conv " + it.layer + ": residual precision mismatch"); return ISEGMI_ERR_STATE; }
        isegmi_conv_desc& d = ds[i];
        memset(&d, 0, sizeof(d));
        d.N = it.in.N; d.H = it.in.H; d.W = it.in.W; d.Cin = it.in.C; d.Cout = L->Cout; d.R = L->R; d.S = L->S; d.stride = it.stride; d.pad = it.pad; d.act = it.act;
        const int Ho = (d.H + 2 * d.pad - d.R) / d.stride + 1, Wo = (d.W + 2 * d.pad - d.S) / d.stride + 1;
        if (it.dst) {
            d.out_div = it.out_div; d.out_img_stride = it.out_img_stride; d.out_pix_stride = it.out_pix_stride;
            out[i] = (float*)it.dst;
        } else {
            int rc = eng_act(e, it.out_name, d.N, Ho, Wo, L->Cout, it.out, 0);
            if (rc) return rc;
            out[i] = it.out->d;
        }
        dp[i] = &d; in[i] = it.in.d; w[i] = (const float*)L->d_w; sc[i] = L->d_scale; sh[i] = L->d_shift; rs[i] = it.residual ? it.residual->d : nullptr;
        fl += 2.0 * d.N * Ho * Wo * (double)d.Cout * d.R * d.S * d.Cin;
        M[i] = Ho * Wo * d.N;
        if (i < 3) label += (i ? " " : "") + it.layer;
    }
    label += n > 3 ? " ... x" + std::to_string(n) + "]" : "]";
    ConvScope cs(e);
    for (int i = 0; i < n; ++i)
        cs.trace(items[i].layer, i == 0 ? ".group" : ".grouped", ds[i].N, ds[i].H, ds[i].W, ds[i].Cin, ds[i].Cout, ds[i].R, ds[i].stride, M[i], rs[i] != nullptr);
    TRY(conv2d_group_launch(n, dp.data(), in.data(), w.data(), sc.data(), sh.data(), rs.data(), out.data(), e.cur));
    cs.done(fl, "%s [%d convolutions, one launch]", label.c_str(), n);
    return ISEGMI_OK;
}

// fp16 bottleneck `block` (conv1 / conv2 / conv3 [/ downsample.0] of an upstream-named ResNet block, stride 1) as ONE launch of the fused kernel
// (csrc/bottleneck_f16.hip) when the block's shape has one: identity blocks of res2 / res3, and -- `first` -- the first block of res2 with its
// projection shortcut.  *fused tells the caller whether it ran (else: three or four eng_conv calls).
int eng_bottleneck_f16(Engine& e, const std::string& block, const Tensor& x, bool first, const std::string& out_name, Tensor* out, bool* fused) {
    *fused = false;
    const float mode = e.param("fused_bottleneck", 1.0f);  // 1: every block that has a fused kernel (default); 2: identity blocks only; 0: none (A/B)
    if (x.dt != 1 || mode == 0.0f || (first && mode == 2.0f)) return ISEGMI_OK;
    auto c1 = e.convs.find(block + ".conv1"), c2 = e.convs.find(block + ".conv2"), c3 = e.convs.find(block + ".conv3"), cd = e.convs.find(block + ".downsample.0");
    if (c1 == e.convs.end() || c2 == e.convs.end() || c3 == e.convs.end() || (first && cd == e.convs.end())) return ISEGMI_OK;
    const ConvLayer &L1 = c1->second, &L2 = c2->second, &L3 = c3->second;
    const ConvLayer* LD = first ? &cd->second : nullptr;
    const int Cmid = L1.Cout, Cout = L3.Cout;
    if (!(L1.f16 && L2.f16 && L3.f16) || L1.Cin != x.C || Cout != 4 * Cmid || L2.Cin != Cmid || L2.Cout != Cmid || L3.Cin != Cmid || L1.R != 1 || L2.R != 3 ||
        L2.S != 3 || L3.R != 1 || !L1.d_scale || !L1.d_shift || !L2.d_scale || !L2.d_shift || !L3.d_scale || !L3.d_shift)
        return ISEGMI_OK;
    if (first) {
        if (!LD->f16 || LD->Cin != x.C || LD->Cout != Cout || LD->R != 1 || !LD->d_scale || !LD->d_shift || !bottleneck_f16_ds_supported(x.C, Cmid)) return ISEGMI_OK;
    } else if (Cout != x.C || !bottleneck_f16_supported(x.C, Cmid)) return ISEGMI_OK;
    if ((int64_t)x.N * x.H * x.W * Cout * 2 >= (1ll << 31)) return ISEGMI_OK;
    int rc = eng_act(e, out_name, x.N, x.H, x.W, Cout, out, 1);
    if (rc) return rc;
    if ((const void*)out->d == (const void*)x.d) { set_error("bottleneck " + block + ": in-place"); return ISEGMI_ERR_STATE; }
    isegmi_bottleneck_desc d;
    memset(&d, 0, sizeof(d));
    d.N = x.N; d.H = x.H; d.W = x.W; d.Cin = x.C; d.Cmid = Cmid;
    ConvScope cs(e);
    const int M = x.N * x.H * x.W;
    cs.trace(block, ".fused", x.N, x.H, x.W, x.C, Cout, 3, 1, M, true);
    TRY(bottleneck_f16_launch(&d, x.d, L1.d_w, L1.d_scale, L1.d_shift, L2.d_w, L2.d_scale, L2.d_shift, L3.d_w, L3.d_scale, L3.d_shift,
                               first ? LD->d_w : nullptr, first ? LD->d_scale : nullptr, first ? LD->d_shift : nullptr, out->d, e.cur));
    // algorithmic FLOPs of the convolutions the launch stands for (the halo the fused kernel recomputes for conv1 is not counted)
    cs.done(2.0 * M * ((double)x.C * Cmid + 9.0 * Cmid * Cmid + (double)Cmid * Cout + (first ? (double)x.C * Cout : 0.0)),
            "%s.fused [M=%d Cin=%d Cmid=%d Cout=%d 1x1+3x3+1x1%s]", block.c_str(), M, x.C, Cmid, Cout, first ? "+proj" : "");
    *fused = true;
    return ISEGMI_OK;
}

// FPN top-down step under fp16: out = lateral1x1(x) + nearest2x(coarse) as ONE launch (UP2X residual mode of the persistent conv kernel); bit-identical to the
// lateral conv followed by nearest2x_add_f16.  *merged = false (nothing launched) with `fused_fpn_merge` 0 or a forced conv tile.
int eng_conv_up2x_f16(Engine& e, const std::string& layer, const Tensor& x, const Tensor& coarse, const std::string& out_name, Tensor* out, bool* merged) {
    *merged = false;
    if (x.dt != 1 || coarse.dt != 1 || e.param("fused_fpn_merge", 1.0f) == 0.0f || e.param("conv_tile", 0) != 0.0f) return ISEGMI_OK;
    auto it = e.convs.find(layer);
    if (it == e.convs.end()) return ISEGMI_OK;
    const ConvLayer& L = it->second;
    if (!L.f16 || L.Cin != x.C || L.R != 1 || L.S != 1 || L.Cout != coarse.C || L.Cout % 8 != 0 || x.W < 8 || coarse.N != x.N) return ISEGMI_OK;
    int rc = eng_act(e, out_name, x.N, x.H, x.W, L.Cout, out, 1);
    if (rc) return rc;
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = x.N; d.H = x.H; d.W = x.W; d.Cin = x.C; d.Cout = L.Cout; d.R = 1; d.S = 1; d.stride = 1; d.pad = 0; d.act = 0;
    ConvScope cs(e);
    const int M = x.N * x.H * x.W;
    cs.trace(layer, ".up2x", x.N, x.H, x.W, x.C, L.Cout, 1, 1, M, true);
    TRY(conv2d_f16_up2x_launch(&d, x.d, L.d_w, L.d_scale, L.d_shift, coarse.d, coarse.H, coarse.W, out->d, e.cur));
    cs.done(2.0 * M * (double)x.C * L.Cout, "%s.up2x [M=%d K=%d Cout=%d 1x1/1 + nearest-2x top-down add]", layer.c_str(), M, x.C, L.Cout);
    *merged = true;
    return ISEGMI_OK;
}

// RPNHead under fp16 (`t = relu(conv3x3(x)); head = cls_bbox(t)`) as ONE launch where the 3x3 runs on the 192 x 256 row-strip tile (csrc/conv_mfma_f16.hip,
// conv_f16_epilogue_head): t stays in LDS.  *fused = false (nothing launched) for levels too small for that tile, or with `fused_rpn_head` 0.
int eng_rpn_head_f16(Engine& e, const std::string& conv, const std::string& headl, const Tensor& x, const std::string& out_name, Tensor* out, bool* fused) {
    *fused = false;
    if (x.dt != 1 || e.param("fused_rpn_head", 1.0f) == 0.0f || e.param("conv_tile", 0) != 0.0f) return ISEGMI_OK;
    auto ic = e.convs.find(conv), ih = e.convs.find(headl);
    if (ic == e.convs.end() || ih == e.convs.end()) return ISEGMI_OK;
    const ConvLayer &L = ic->second, &H = ih->second;
    if (!L.f16 || !H.f16 || L.Cin != x.C || L.R != 3 || L.S != 3 || L.Cout != 256 || H.Cin != 256 || H.R != 1 || H.S != 1 || H.Cout > 32) return ISEGMI_OK;
    int rc = eng_act(e, out_name, x.N, x.H, x.W, H.Cout, out, 0);
    if (rc) return rc;
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = x.N; d.H = x.H; d.W = x.W; d.Cin = x.C; d.Cout = 256; d.R = 3; d.S = 3; d.stride = 1; d.pad = 1; d.act = 1;
    ConvScope cs(e);
    TRY(conv2d_f16_head_launch(&d, x.d, L.d_w, L.d_scale, L.d_shift, H.d_w, H.d_scale, H.d_shift, H.Cout, out->d, fused, e.cur));
    if (!*fused) return ISEGMI_OK;
    const int M = x.N * x.H * x.W;
    cs.trace(conv + "+" + headl, ".fused", x.N, x.H, x.W, x.C, H.Cout, 3, 1, M, false);
    // both convolutions' algorithmic FLOPs
    cs.done(2.0 * M * (9.0 * x.C * 256 + 256.0 * H.Cout), "%s+%s.fused [M=%d K=%d Cout=256 3x3/1 + 1x1 -> %d]", conv.c_str(), headl.c_str(), M, 9 * x.C, H.Cout);
    return ISEGMI_OK;
}

// fp16 stem conv + BN + ReLU + 3x3/2 max-pool as ONE launch (csrc/stem_pool_f16.hip); *fused = false (nothing launched) when the layer is not the 64-channel
// stem or `fused_stem` is 0 (A/B against the two launches)
int eng_stem_pool_f16(Engine& e, const std::string& layer, const Tensor& halo, int H, int W, const std::string& out_name, Tensor* out, bool* fused) {
    *fused = false;
    if (e.param("fused_stem", 1.0f) == 0.0f || halo.dt != 1) return ISEGMI_OK;
    auto it = e.convs.find(layer);
    if (it == e.convs.end()) return ISEGMI_OK;
    const ConvLayer& L = it->second;
    if (!L.f16 || L.Cin != 4 || L.R != 7 || L.S != 7 || !stem_pool_f16_supported(L.Cout) || !L.d_scale || !L.d_shift) return ISEGMI_OK;
    const int Hc = (H + 6 - 7) / 2 + 1, Wc = (W + 6 - 7) / 2 + 1, Hp = (Hc + 2 - 3) / 2 + 1, Wp = (Wc + 2 - 3) / 2 + 1;
    int rc = eng_act(e, out_name, halo.N, Hp, Wp, L.Cout, out, 1);
    if (rc) return rc;
    ConvScope cs(e);
    const int M = halo.N * Hc * Wc;
    cs.trace(layer, ".fused", halo.N, H, W, 4, L.Cout, 7, 2, M, true);
    TRY(stem_pool_f16_launch(halo.N, H, W, halo.d, L.d_w, L.d_scale, L.d_shift, out->d, 0, e.cur));
    // the convolution's algorithmic FLOPs (7 x 7 x 3 taps), as the unfused layer counts them
    cs.done(2.0 * M * 147.0 * L.Cout, "%s.fused [M=%d K=196 Cout=%d 7x7/2 + maxpool 3x3/2]", layer.c_str(), M, L.Cout);
    *fused = true;
    return ISEGMI_OK;
}

// fp16 stem: `halo` is the [N][H+6][(W+7)&~1][4] fp16 image of pad_c3_to_f16_halo; H, W the image size
int eng_conv_stem_f16(Engine& e, const std::string& layer, const Tensor& halo, int H, int W, const std::string& out_name, Tensor* out) {
    const ConvLayer* L;
    int rc = find_conv(e, layer, &L);
    if (rc) return rc;
    if (!L->f16 || L->Cin != 4 || L->R != 7 || L->S != 7 || halo.dt != 1) { set_error("conv " + layer + ": not an fp16 stem"); return ISEGMI_ERR_STATE; }
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    rc = eng_act(e, out_name, halo.N, Ho, Wo, L->Cout, out, 1);
    if (rc) return rc;
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = halo.N; d.H = H; d.W = W; d.Cin = 4; d.Cout = L->Cout; d.R = 7; d.S = 7; d.stride = 2; d.pad = 3; d.act = 1;
    return timed_conv(e, layer, &d, halo.d, L, nullptr, out->d, false);
}

int eng_next_event(Engine& e, hipEvent_t* ev) {
    if (e.ev_pool.empty()) {
        e.ev_pool.resize(128);
        for (auto& x : e.ev_pool) HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    }
    *ev = e.ev_pool[e.ev_next++ % e.ev_pool.size()];
    return ISEGMI_OK;
}
int eng_fork(Engine& e, int k) {
    if (!e.multi_stream) return ISEGMI_OK;
    hipEvent_t ev;
    int rc = eng_next_event(e, &ev);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev, e.stream));
    HIP_TRY(hipStreamWaitEvent(e.side[k], ev, 0));
    return ISEGMI_OK;
}
int eng_join(Engine& e, int k) {
    if (!e.multi_stream) return ISEGMI_OK;
    hipEvent_t ev;
    int rc = eng_next_event(e, &ev);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev, e.side[k]));
    HIP_TRY(hipStreamWaitEvent(e.stream, ev, 0));
    return ISEGMI_OK;
}

// End of a forward's tail section.  Eager: leave the tail stream running (the next forward overlaps with it) and record
// the WAR fence.  Under graph capture: join the tail back into the main stream so the capture ends on one stream.
int eng_tail_end(Engine& e) {
    if (!e.multi_stream) return ISEGMI_OK;
    if (e.capturing) {
        hipEvent_t ev;
        int rc = eng_next_event(e, &ev);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev, e.tail));
        HIP_TRY(hipStreamWaitEvent(e.stream, ev, 0));
        return ISEGMI_OK;
    }
    HIP_TRY(hipEventRecord(e.tail_done, e.tail));
    e.tail_pending = true;
    return ISEGMI_OK;
}

// Input slot rule: a front-end write into an input slot (upload_async, and the preprocess kernel behind an upload_u8_async) must follow the LAST READ
// of that slot by every forward enqueued so far.  The two lanes' forwards share no stream, so each lane records its own event right after the one
// kernel of its forward that reads the caller's input, and isegmi_engine_upload_async makes the copy stream wait on every lane's pending event
// before it writes (conservative: it does not track which slot a lane read; the event sits behind the first kernel of a forward, so the wait is short).
int eng_input_consumed(Engine& e) {
    if (e.capturing || e.in_done[e.lane] == nullptr) return ISEGMI_OK;
    HIP_TRY(hipEventRecord(e.in_done[e.lane], e.cur));
    e.in_pending[e.lane] = true;
    return ISEGMI_OK;
}

// The consumer of an uploaded buffer (the front-end kernel for a uint8 staging buffer, the forward for an input slot) waits for the
// upload_async / front-end launches that filled [d_ptr, d_ptr + bytes) -- and only for those.
int eng_wait_upload(Engine& e, const void* d_ptr, int64_t bytes, hipStream_t st) {
    const char* p = (const char*)d_ptr;
    const unsigned bit = (st != nullptr && st == e.lane_stream[1]) ? 2u : 1u;   // the lane whose main stream waits
    for (auto& u : e.uploads)
        if (!(u.waited & bit) && p < u.dst + u.bytes && u.dst < p + bytes) { HIP_TRY(hipStreamWaitEvent(st, u.done, 0)); u.waited |= bit; }
    return ISEGMI_OK;
}

// Registers "stream st (the copy stream; the main stream for a front-end launch there) has, up to here, written [d_dst, d_dst + bytes)": one completion
// event per destination.  `ordered`: the lanes whose main stream is already behind the write (bits as in Upload::waited).
static int eng_note_upload(Engine& e, const void* d_dst, int64_t bytes, hipStream_t st = nullptr, unsigned ordered = 0u) {
    Engine::Upload* u = nullptr;
    for (auto& x : e.uploads) if (x.dst == (const char*)d_dst) u = &x;
    if (!u) {
        if (e.uploads.size() >= 64) {  // destinations come and go (staging buffers are re-allocated when they grow): recycle a consumed entry
            for (auto& x : e.uploads) if (e.consumed(x)) { u = &x; break; }
            if (u == nullptr) { set_error("more than 64 upload destinations with unconsumed uploads"); return ISEGMI_ERR_STATE; }
        } else {
            e.uploads.emplace_back();
            u = &e.uploads.back();
            HIP_TRY(hipEventCreateWithFlags(&u->done, hipEventDisableTiming));
        }
        u->dst = (const char*)d_dst;
    }
    u->bytes = bytes;
    HIP_TRY(hipEventRecord(u->done, st ? st : e.copy));
    u->waited = ordered;
    return ISEGMI_OK;
}

hipStream_t eng_results_stream(Engine& e) { return (e.multi_stream && e.tail_pending) ? e.tail : e.stream; }

int eng_stage_small(Engine& e, const void* h_src, size_t bytes, void* d_dst, hipStream_t st) {
    if (bytes > (size_t)Engine::PIN_SLOT_BYTES) { set_error("eng_stage_small: array larger than a pinned ring slot"); return ISEGMI_ERR_ARG; }
    if (e.capturing) { set_error("host array staged during graph capture"); return ISEGMI_ERR_STATE; }
    if (e.pin_ring == nullptr) HIP_TRY(hipHostMalloc((void**)&e.pin_ring, (size_t)Engine::PIN_SLOTS * Engine::PIN_SLOT_BYTES, hipHostMallocDefault));
    const int s = e.pin_next++ % Engine::PIN_SLOTS;
    if (e.pin_ev[s] == nullptr) HIP_TRY(hipEventCreateWithFlags(&e.pin_ev[s], hipEventDisableTiming));
    if (e.pin_used[s]) HIP_TRY(hipEventSynchronize(e.pin_ev[s]));  // the copy that last used this slot (PIN_SLOTS stagings ago) has long finished
    char* slot = e.pin_ring + (size_t)s * Engine::PIN_SLOT_BYTES;
    memcpy(slot, h_src, bytes);
    HIP_TRY(hipMemcpyAsync(d_dst, slot, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e.pin_ev[s], st));
    e.pin_used[s] = true;
    return ISEGMI_OK;
}

void eng_graph_reset(Engine& e) {
    for (auto& kv : e.graphs) (void)hipGraphExecDestroy(kv.second);
    e.graphs.clear();
    e.graph_warm.clear();
}

// Run `body` (a forward's enqueue code) eagerly, or -- with the "graph" param set -- capture it on the second call with the
// same key and replay the instantiated graph from then on.  The first call stays eager so that every buffer exists.
int eng_graph_run(Engine& e, const std::string& key, const std::function<int()>& body) {
    const bool want = e.param("graph", 0.0f) != 0.0f && e.multi_stream && !e.timing && !e.conv_timing;
    if (!want) return body();
    auto it = e.graphs.find(key);
    if (it == e.graphs.end()) {
        int& warm = e.graph_warm[key];
        if (warm == 0) { warm = 1; return body(); }
        if (warm < 0) return body();  // capture failed before: stay eager
        if (e.tail_pending) { HIP_TRY(hipStreamWaitEvent(e.stream, e.tail_done, 0)); e.tail_pending = false; }
        HIP_TRY(hipStreamBeginCapture(e.stream, hipStreamCaptureModeRelaxed));
        e.capturing = true;
        const int rc = body();
        e.capturing = false;
        hipGraph_t g = nullptr;
        const hipError_t er = hipStreamEndCapture(e.stream, &g);
        if (rc != ISEGMI_OK || er != hipSuccess || g == nullptr) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            warm = -1;
            ++e.graph_failures;
            for (int k = 0; k < 3; ++k) (void)hipStreamSynchronize(e.side[k]);
            (void)hipStreamSynchronize(e.tail);
            return body();
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess) { (void)hipGetLastError(); warm = -1; ++e.graph_failures; return body(); }
        it = e.graphs.emplace(key, exec).first;
        ++e.graph_captures;
    }
    if (e.tail_pending) { HIP_TRY(hipStreamWaitEvent(e.stream, e.tail_done, 0)); e.tail_pending = false; }
    HIP_TRY(hipGraphLaunch(it->second, e.stream));
    ++e.graph_replays;
    // eng_input_consumed() is skipped under capture and never runs on a replay: the end of the graph is the (conservative) point
    // after which the next upload_async may overwrite the input / staging buffer
    if (e.in_done[0]) { HIP_TRY(hipEventRecord(e.in_done[0], e.stream)); e.in_pending[0] = true; }
    return ISEGMI_OK;
}

void eng_mark(Engine& e, const char* name) {
    if (!e.timing) return;
    StageTime s;
    s.name = name;
    if (hipEventCreate(&s.ev) != hipSuccess) return;
    (void)hipEventRecord(s.ev, e.cur ? e.cur : e.stream);
    e.marks.push_back(s);
}

static void collect_times(Engine& e) {
    for (size_t i = 0; i < e.conv_evs.size(); ++i) {
        auto& pr = e.conv_evs[i];
        float ms = 0;
        (void)hipEventElapsedTime(&ms, pr.first, pr.second);
        auto& acc = e.conv_layers[e.conv_ev_info[i].first];
        acc.first += e.conv_ev_info[i].second;
        acc.second += ms;
        e.conv_ms += ms;
        e.conv_launches += 1;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    e.conv_evs.clear();
    e.conv_ev_info.clear();
    e.conv_flops += e.conv_flops_pending;
    e.conv_flops_pending = 0;
    e.last_times.clear();
    if (!e.timing || e.marks.empty()) return;
    (void)hipEventSynchronize(e.marks.back().ev);
    for (size_t i = 1; i < e.marks.size(); ++i) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e.marks[i - 1].ev, e.marks[i].ev);
        e.last_times.push_back({e.marks[i].name, ms});
    }
    for (auto& m : e.marks) (void)hipEventDestroy(m.ev);
    e.marks.clear();
}

}  // namespace isegmi

using namespace isegmi;

// ---- which of the engine's streams share an in-order hardware queue?  The runtime folds a process's streams onto GPU_MAX_HW_QUEUES (4) queues by
// what the process has created so far; two streams of one queue serialise although the stream-level program says they may overlap (DESIGN section 4,
// "Streams against four in-order hardware queues").  Probe: a one-wave kernel spins ~40 us on stream a, an empty kernel follows on stream b; b's
// kernel ends before a's only if the two sit on different queues.  Streams are classed against one representative per class found so far.
namespace {
__global__ void probe_spin_kernel(long long cycles, int* sink) {
    const long long t0 = clock64();
    while (clock64() - t0 < cycles) {}
    if (sink && cycles < 0) *sink = 1;
}
__global__ void probe_nop_kernel(int* sink) { if (sink && sink[0] == 0x7fffffff) sink[0] = 0; }

int same_queue_once(hipStream_t a, hipStream_t b, bool* same) {
    hipEvent_t s, ea, eb;
    HIP_TRY(hipEventCreate(&s)); HIP_TRY(hipEventCreate(&ea)); HIP_TRY(hipEventCreate(&eb));
    HIP_TRY(hipStreamSynchronize(a)); HIP_TRY(hipStreamSynchronize(b));
    HIP_TRY(hipEventRecord(s, a));
    hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(64), 0, a, 100000LL, (int*)nullptr);   // ~40-50 us at 2.1-2.4 GHz
    HIP_TRY(hipEventRecord(ea, a));
    hipLaunchKernelGGL(probe_nop_kernel, dim3(1), dim3(64), 0, b, (int*)nullptr);
    HIP_TRY(hipEventRecord(eb, b));
    HIP_TRY(hipStreamSynchronize(a)); HIP_TRY(hipStreamSynchronize(b));
    float ta = 0.0f, tb = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ta, s, ea));
    HIP_TRY(hipEventElapsedTime(&tb, s, eb));
    *same = tb > 0.7f * ta;   // b's empty kernel finished only when the spin had: it queued behind it
    (void)hipEventDestroy(s); (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    return ISEGMI_OK;
}

// A stream's FIRST launch pays for the lazy creation of its queue state (longer than the spin: a fresh stream then looks as if it had waited), and a
// launch can be late for other reasons: both streams are warmed up first, and "same queue" needs two probes out of two to say so.
int same_queue(hipStream_t a, hipStream_t b, bool* same) {
    hipLaunchKernelGGL(probe_nop_kernel, dim3(1), dim3(64), 0, a, (int*)nullptr);
    hipLaunchKernelGGL(probe_nop_kernel, dim3(1), dim3(64), 0, b, (int*)nullptr);
    HIP_TRY(hipStreamSynchronize(a)); HIP_TRY(hipStreamSynchronize(b));
    bool s1 = false, s2 = false;
    int rc = same_queue_once(a, b, &s1);
    if (rc) return rc;
    if (s1) { rc = same_queue_once(a, b, &s2); if (rc) return rc; }
    *same = s1 && s2;
    return ISEGMI_OK;
}
}  // namespace

// ---- process-wide pool of stream sets.  An engine BORROWS its ten streams (main, 3 side, tail, heads, 3 heads-side, copy) and hands them back
// when it is destroyed; the next engine of the process gets the very same streams.  Why not create / destroy per engine: the runtime places a
// new stream on one of its four in-order hardware queues by what the process has created (and destroyed) so far, and an engine's speed depends on
// which of its streams end up sharing a queue -- Mask R-CNN bs=2 ran 220.0 img/s as the first engine of a process and 204.8 as the second, after a
// Yolact engine had been created and closed (tools/second_engine_probe.py; the default bench.py line's embedded configs[2] figure was such a second
// engine).  With the pool every engine that follows a closed one sees the first one's placement.  Engines alive at the same time get sets of their own.
// Round 4: the ten streams are no longer "the next ten the runtime hands out".  Which hardware queue a new stream lands on depends on every
// stream the process created before (a foreign HIP library, another engine), and the placement decides the throughput: measured with the probe
// above (tools/stream_layout_probe.py, Yolact bs 8): 986 img/s whenever the MAIN stream's queue carries neither the tail, nor the heads, nor the
// copy stream and the tail's queue carries neither of the other two; 922 with heads + copy on main's queue (one or three foreign streams created
// first), 913 with the tail on it (four or five).  So a set is built from up to 24 CANDIDATE streams whose queues are probed, and the roles are
// dealt by queue class to reproduce the layout a fresh process gets (classes A main / side0 / heads-side1, B side2 / tail / heads-side2,
// C side1 / heads / copy, D heads-side0); candidates not needed stay idle in the set (destroying them would shift the next set's placement).
namespace {
struct StreamSet {
    int dev = 0; bool used = false; hipStream_t s[10] = {nullptr}; std::vector<hipStream_t> spare; int placed = 0;
    hipStream_t lane1[4] = {nullptr};   // the second backbone lane's main + three side streams (deal_lane_streams), dealt on first demand
    int lane_state = 0;                 // as Engine::lane_state
};
std::mutex g_sets_mu;
std::vector<StreamSet*> g_sets;

int acquire_streams(StreamSet** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_sets_mu);
    for (StreamSet* ss : g_sets)
        if (!ss->used && ss->dev == dev) { ss->used = true; *out = ss; return ISEGMI_OK; }
    StreamSet* ss = new StreamSet();
    ss->dev = dev;
    std::vector<hipStream_t> cand;
    std::vector<int> cls;            // queue class of each candidate (0 = the first candidate's queue)
    std::vector<int> rep;            // one candidate per class
    auto fail = [&](hipError_t er) {
        for (hipStream_t c : cand) (void)hipStreamDestroy(c);
        delete ss;
        set_error(std::string("hipStreamCreate: ") + hipGetErrorString(er));
        return ISEGMI_ERR_HIP;
    };
    // classes in order of discovery: A = the main stream's queue, B, C, D the next three.  Role -> preferred classes (first available wins):
    //   main A | tail B | heads C, copy C (never A, never the tail's) | side0 -- the backbone's projection shortcuts -- D or A, never behind the tail
    //   or the heads phase (942 / 920 img/s when it was; 988 on D, 979 on A) | side1 C, side2 B, heads-side D / A / B as in a fresh process
    static const int pref[10][3] = {{0, 0, 0}, {3, 0, -1}, {2, 3, -1}, {1, 3, -1}, {1, -1, -1}, {2, -1, -1}, {3, 0, -1}, {0, 3, -1}, {1, 3, -1}, {2, -1, -1}};
    int prefv[10][3];
    memcpy(prefv, pref, sizeof(prefv));
    if (const char* ov = getenv("ISEGMI_STREAM_LAYOUT")) {   // dev: ten class digits (0 = A .. 3 = D), role order main side0-2 tail heads hs0-2 copy
        for (int i = 0; i < 10 && ov[i] >= '0' && ov[i] <= '3'; ++i) { prefv[i][0] = ov[i] - '0'; prefv[i][1] = prefv[i][2] = -1; }
    }
    const bool probe = getenv("ISEGMI_STREAM_PLACEMENT") == nullptr || atoi(getenv("ISEGMI_STREAM_PLACEMENT")) != 0;  // 0: the round-3 behaviour (A/B)
    const int need[4] = {1, 4, 4, 4};   // (A often gets no second stream from the runtime: side0 / heads-side1 then take D)
    int have[4] = {0, 0, 0, 0};
    const int max_cand = probe ? 24 : 10;
    while ((int)cand.size() < max_cand) {
        hipStream_t st = nullptr;
        hipError_t er = cand.empty() ? hipStreamCreate(&st) : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (er != hipSuccess) return fail(er);
        cand.push_back(st);
        int c = -1;
        if (probe) {
            for (size_t r = 0; r < rep.size() && c < 0; ++r) {
                bool same = false;
                if (same_queue(cand[rep[r]], st, &same) != ISEGMI_OK) return fail(hipErrorUnknown);
                if (same) c = (int)r;
            }
            if (c < 0) { c = (int)rep.size(); rep.push_back((int)cand.size() - 1); }
        } else {
            c = 0;
        }
        cls.push_back(c);
        if (c < 4) ++have[c];
        if (cand.size() >= 10 && (!probe || (have[0] >= need[0] && have[1] >= need[1] && have[2] >= need[2] && have[3] >= need[3]))) break;
    }
    // deal the roles: a candidate of a preferred class if there is one left, else any left-over candidate (fewer than four queues, or an odd
    // distribution: correct either way, only the overlap differs)
    std::vector<bool> taken(cand.size(), false);
    ss->placed = 1;
    for (int i = 0; i < 10; ++i) {
        int pick = -1;
        if (i == 0) pick = 0;       // the one blocking stream is the main stream
        for (int q = 0; q < 3 && pick < 0 && probe; ++q)
            for (size_t j = 1; j < cand.size() && pick < 0; ++j) if (!taken[j] && prefv[i][q] >= 0 && cls[j] == prefv[i][q]) pick = (int)j;
        for (size_t j = 1; j < cand.size() && pick < 0; ++j) if (!taken[j]) { pick = (int)j; if (probe) ss->placed = 0; }
        taken[pick] = true;
        ss->s[i] = cand[pick];
    }
    for (size_t j = 0; j < cand.size(); ++j) if (!taken[j]) ss->spare.push_back(cand[j]);
    ss->used = true;
    g_sets.push_back(ss);
    *out = ss;
    return ISEGMI_OK;
}

// The second backbone lane ("step_overlap") needs a main stream whose hardware queue carries neither lane 0's main stream nor the tail (two backbones on
// one in-order queue would simply run one after the other; behind the tail it would wait for every Detect chain), and preferably not the heads stream
// either.  With four queues that is the fourth class of the partition above (D), which otherwise carries only heads-side streams that are idle at the
// bench batch.  It is taken from the set's idle candidates -- their queues are probed against the three live roles -- and only if none qualifies are up
// to eight further streams created and probed.  No such queue (a runtime that hands out fewer distinct queues than the partition needs): lane_state -1,
// the engine stays on one lane and says so (isegmi_engine_lane_layout) rather than share a queue.  Lane 1's side streams: side0 on its own main's queue
// or lane 0's main's, side1 / side2 on the queues of lane 0's side1 / side2 where a candidate is left, else any idle candidate, else a new stream.
int deal_lane_streams(StreamSet* ss) {
    if (ss->lane_state != 0) return ISEGMI_OK;
    auto qualifies = [&](hipStream_t c, int* q) -> int {   // *q: 0 no, 1 shares the heads stream's queue, 2 free of all three
        bool same = false;
        *q = 0;
        int rc = same_queue(ss->s[0], c, &same);
        if (rc || same) return rc;
        rc = same_queue(ss->s[4], c, &same);
        if (rc || same) return rc;
        rc = same_queue(ss->s[5], c, &same);
        if (rc) return rc;
        *q = same ? 1 : 2;
        return ISEGMI_OK;
    };
    int pick = -1, second = -1;
    for (size_t j = 0; j < ss->spare.size() && pick < 0; ++j) {
        int q = 0;
        int rc = qualifies(ss->spare[j], &q);
        if (rc) return rc;
        if (q == 2) pick = (int)j;
        else if (q == 1 && second < 0) second = (int)j;
    }
    for (int extra = 0; extra < 8 && pick < 0; ++extra) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        ss->spare.push_back(st);
        int q = 0;
        int rc = qualifies(st, &q);
        if (rc) return rc;
        if (q == 2) pick = (int)ss->spare.size() - 1;
        else if (q == 1 && second < 0) second = (int)ss->spare.size() - 1;
    }
    if (pick < 0) pick = second;
    if (pick < 0) { ss->lane_state = -1; return ISEGMI_OK; }
    ss->lane1[0] = ss->spare[pick];
    ss->spare.erase(ss->spare.begin() + pick);
    for (int k = 0; k < 3; ++k) {
        const hipStream_t want[2] = {k == 0 ? ss->lane1[0] : ss->s[1 + k], k == 0 ? ss->s[0] : nullptr};
        int got = -1;
        for (int w = 0; w < 2 && got < 0 && want[w]; ++w)
            for (size_t j = 0; j < ss->spare.size() && got < 0; ++j) {
                bool same = false;
                int rc = same_queue(want[w], ss->spare[j], &same);
                if (rc) return rc;
                if (same) got = (int)j;
            }
        if (got < 0 && !ss->spare.empty()) got = 0;
        if (got < 0) {
            hipStream_t st = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
                (void)hipGetLastError();
                for (int i = 0; i <= k; ++i) if (ss->lane1[i]) { ss->spare.push_back(ss->lane1[i]); ss->lane1[i] = nullptr; }
                ss->lane_state = -1;
                return ISEGMI_OK;
            }
            ss->lane1[1 + k] = st;
            continue;
        }
        ss->lane1[1 + k] = ss->spare[got];
        ss->spare.erase(ss->spare.begin() + got);
    }
    ss->lane_state = 1;
    return ISEGMI_OK;
}

void release_streams(StreamSet* ss) {
    if (!ss) return;
    for (int i = 0; i < 10; ++i) (void)hipStreamSynchronize(ss->s[i]);
    for (int i = 0; i < 4; ++i) if (ss->lane1[i]) (void)hipStreamSynchronize(ss->lane1[i]);
    std::lock_guard<std::mutex> lk(g_sets_mu);
    ss->used = false;
}
}  // namespace


// queue_class[i] for the engine's ten streams (0 main, 1-3 side, 4 tail, 5 heads, 6-8 heads-side, 9 copy): equal numbers share a hardware queue.
// Call on an idle engine (it synchronises the streams).
extern "C" int isegmi_engine_stream_layout(isegmi_engine* h, int32_t* queue_class, int n) {
    ARG_CHECK(h && queue_class && n >= 10, "stream_layout args");
    StreamSet* ss = (StreamSet*)h->e.stream_set;
    ARG_CHECK(ss, "engine has no streams");
    int reps[10], nrep = 0;
    for (int i = 0; i < 10; ++i) {
        int cls = -1;
        for (int r = 0; r < nrep && cls < 0; ++r) {
            bool same = false;
            int rc = same_queue(ss->s[reps[r]], ss->s[i], &same);
            if (rc) return rc;
            if (same) cls = r;
        }
        if (cls < 0) { cls = nrep; reps[nrep++] = i; }
        queue_class[i] = cls;
    }
    return ISEGMI_OK;
}

// "step_overlap" in force for the next forward?  Yolact fp32, eager multi-stream throughput mode only: off under graph capture / the "graph" latency
// mode (a captured graph keeps its one-lane shape), with multi_stream 0, and under the stage / conv timing modes, whose events must bracket one stream's
// kernels.  The first call that finds it wanted deals lane 1's streams (probes queues: a few ms, once per process and stream set).
static int lanes_active(Engine& e, bool* on) {
    *on = false;
    if (e.kind != 1 || e.fp16 || !e.multi_stream || e.capturing || e.timing || e.conv_timing || e.param("graph", 0.0f) != 0.0f ||
        e.param("step_overlap", STEP_OVERLAP_DEFAULT) == 0.0f)
        return ISEGMI_OK;
    if (e.lane_state == 0) {
        StreamSet* ss = (StreamSet*)e.stream_set;
        {
            std::lock_guard<std::mutex> lk(g_sets_mu);
            int rc = deal_lane_streams(ss);
            if (rc) return rc;
        }
        e.lane_state = ss->lane_state;
        if (e.lane_state == 1) {
            e.lane_stream[1] = ss->lane1[0];
            for (int k = 0; k < 3; ++k) e.lane_side[1][k] = ss->lane1[1 + k];
        }
    }
    *on = e.lane_state == 1;
    return ISEGMI_OK;
}

// Read-out of the backbone lanes ("step_overlap"), n >= 18.  Call on an idle engine (it synchronises the streams, and deals lane 1's when wanted).
//   out[0]     lanes the next forward would alternate over (2, or 1: parameter off / forced off / fallback)
//   out[1]     1 = step_overlap is wanted but the runtime gave lane 1's main stream no queue of its own: the engine FELL BACK to one lane
//   out[2..11] queue classes of the ten roles, as isegmi_engine_stream_layout numbers them
//   out[12..15] queue classes of lane 1's main, side0, side1, side2 in the same numbering (-1: not dealt)
//   out[16]    lanes the LAST forward alternated over; out[17] forwards that ran on lane 1 so far (saturating at INT32_MAX)
extern "C" int isegmi_engine_lane_layout(isegmi_engine* h, int32_t* out, int n) {
    ARG_CHECK(h && out && n >= 18, "lane_layout args");
    Engine& e = h->e;
    StreamSet* ss = (StreamSet*)e.stream_set;
    ARG_CHECK(ss, "engine has no streams");
    bool on = false;
    int rc = lanes_active(e, &on);
    if (rc) return rc;
    out[0] = on ? 2 : 1;
    out[1] = e.lane_state == -1 ? 1 : 0;
    hipStream_t all[14];
    for (int i = 0; i < 10; ++i) all[i] = ss->s[i];
    for (int i = 0; i < 4; ++i) all[10 + i] = e.lane_state == 1 ? ss->lane1[i] : nullptr;
    int reps[14], nrep = 0;
    for (int i = 0; i < 14; ++i) {
        int cls = -1;
        if (all[i] == nullptr) { out[2 + i] = -1; continue; }
        for (int r = 0; r < nrep && cls < 0; ++r) {
            bool same = false;
            rc = same_queue(all[reps[r]], all[i], &same);
            if (rc) return rc;
            if (same) cls = r;
        }
        if (cls < 0) { cls = nrep; reps[nrep++] = i; }
        out[2 + i] = cls;
    }
    out[16] = e.last_lanes;
    out[17] = (int32_t)(e.lane1_forwards > 0x7fffffff ? 0x7fffffff : e.lane1_forwards);
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_create(int model_kind, int max_batch, int H, int W, isegmi_engine** out) {
    ARG_CHECK(out, "null out");
    // 6 is not a kind: tests/test_yolov3_gpu.py pins that isegmi_engine_create refuses it, so ViT took the next number
    ARG_CHECK((model_kind >= 1 && model_kind <= 5) || model_kind == 7, "model_kind: 1 yolact, 2 maskrcnn, 3 pose2seg, 4 retinanet, 5 yolov3, 7 vit");
    ARG_CHECK(model_kind != 5 || (H % 32 == 0 && W % 32 == 0 && H <= 1024 && W <= 1024), "yolov3: canvas sides are multiples of 32 in 32..1024");
    ARG_CHECK(model_kind != 3 || (H == 512 && W == 512), "pose2seg: the input plane is 512 x 512");
    ARG_CHECK(max_batch > 0 && H > 0 && W > 0, "sizes");
    isegmi_engine* h = new isegmi_engine();
    h->e.kind = model_kind; h->e.max_batch = max_batch; h->e.H = H; h->e.W = W;
    StreamSet* ss = nullptr;
    if (acquire_streams(&ss) != ISEGMI_OK) { delete h; return ISEGMI_ERR_HIP; }
    h->e.stream_set = ss;
    h->e.stream = ss->s[0];
    for (int i = 0; i < 3; ++i) h->e.side[i] = ss->s[1 + i];
    h->e.tail = ss->s[4];
    h->e.heads = ss->s[5];
    for (int i = 0; i < 3; ++i) h->e.hside[i] = ss->s[6 + i];
    h->e.copy = ss->s[9];
    h->e.lane_stream[0] = h->e.stream;
    for (int i = 0; i < 3; ++i) h->e.lane_side[0][i] = h->e.side[i];
    hipError_t er = hipEventCreateWithFlags(&h->e.tail_done, hipEventDisableTiming);
    for (int l = 0; l < 2; ++l) {
        if (er == hipSuccess) er = hipEventCreateWithFlags(&h->e.lat_done[l], hipEventDisableTiming);
        if (er == hipSuccess) er = hipEventCreateWithFlags(&h->e.in_done[l], hipEventDisableTiming);
    }
    if (er == hipSuccess) er = hipEventCreateWithFlags(&h->e.heads_done, hipEventDisableTiming);
    if (er != hipSuccess) { set_error(std::string("engine events: ") + hipGetErrorString(er)); release_streams(ss); delete h; return ISEGMI_ERR_HIP; }
    h->e.cur = h->e.stream;
    *out = h;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_destroy(isegmi_engine* h) {
    if (!h) return ISEGMI_OK;
    Engine& e = h->e;
    if (e.stream_set) for (int i = 0; i < 10; ++i) (void)hipStreamSynchronize(((StreamSet*)e.stream_set)->s[i]);  // nothing of this engine is in flight any more
    for (int i = 0; i < 4; ++i) if (e.stream_set && ((StreamSet*)e.stream_set)->lane1[i]) (void)hipStreamSynchronize(((StreamSet*)e.stream_set)->lane1[i]);
    eng_graph_reset(e);
    if (e.heads) { (void)hipStreamSynchronize(e.heads); }
    if (e.tail) (void)hipStreamSynchronize(e.tail);
    if (e.tail_done) (void)hipEventDestroy(e.tail_done);
    for (int l = 0; l < 2; ++l) if (e.lat_done[l]) (void)hipEventDestroy(e.lat_done[l]);
    if (e.heads_done) (void)hipEventDestroy(e.heads_done);
    if (e.copy) (void)hipStreamSynchronize(e.copy);
    for (int l = 0; l < 2; ++l) if (e.in_done[l]) (void)hipEventDestroy(e.in_done[l]);
    for (auto& u : e.uploads) if (u.done) (void)hipEventDestroy(u.done);
    for (int i = 0; i < 2; ++i) if (e.dl_done[i]) (void)hipEventDestroy(e.dl_done[i]);
    for (int i = 0; i < Engine::PIN_SLOTS; ++i) if (e.pin_ev[i]) (void)hipEventDestroy(e.pin_ev[i]);
    if (e.pin_ring) (void)hipHostFree(e.pin_ring);
    for (auto& ev : e.step_marks) (void)hipEventDestroy(ev);
    for (auto& kv : e.p2s_kpts_read) (void)hipEventDestroy(kv.second);
    for (auto& kv : e.convs) {
        if (kv.second.view) continue;
        (void)hipFree(kv.second.d_w); if (kv.second.d_scale) (void)hipFree(kv.second.d_scale); if (kv.second.d_shift) (void)hipFree(kv.second.d_shift);
    }
    for (auto& kv : e.tensors) (void)hipFree(kv.second.d);
    for (auto& kv : e.bufs) (void)hipFree(kv.second.d);
    for (auto& ev : e.ev_pool) (void)hipEventDestroy(ev);
    release_streams((StreamSet*)e.stream_set);  // back to the process-wide pool (synchronised there), not destroyed
    delete h;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_set_param(isegmi_engine* h, const char* name, float value) {
    ARG_CHECK(h && name, "null");
    if (std::string(name) != "graph") eng_graph_reset(h->e);  // kernel arguments are baked into captured graphs
    h->e.params[name] = value;
    if (std::string(name) == "timing") h->e.timing = value != 0.0f;
    if (std::string(name) == "conv_timing") h->e.conv_timing = value != 0.0f;
    if (std::string(name) == "op_timing") h->e.op_timing = value != 0.0f;
    if (std::string(name) == "conv_trace") h->e.conv_trace = value != 0.0f;
    if (std::string(name) == "multi_stream") h->e.multi_stream = value != 0.0f;
    if (std::string(name) == "fp16") h->e.fp16 = value != 0.0f;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_get_param(isegmi_engine* h, const char* name, float default_value, float* value, int32_t* is_set) {
    ARG_CHECK(h && name && value, "null");
    auto it = h->e.params.find(name);
    *value = it == h->e.params.end() ? default_value : it->second;
    if (is_set) *is_set = it == h->e.params.end() ? 0 : 1;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_graph_stats(isegmi_engine* h, int64_t* captures, int64_t* replays, int64_t* failures) {
    ARG_CHECK(h, "null");
    if (captures) *captures = h->e.graph_captures;
    if (replays) *replays = h->e.graph_replays;
    if (failures) *failures = h->e.graph_failures;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_set_conv(isegmi_engine* h, const char* name, int Cout, int R, int S, int Cin, const float* h_w_krsc,
                                      const float* h_scale, const float* h_shift) {
    ARG_CHECK(h && name && h_w_krsc, "null");
    ARG_CHECK(strchr(name, '[') == nullptr, "set_conv: '[' in a layer name (row-range views are the engine's)");
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = 1; d.H = R; d.W = S; d.Cin = Cin; d.Cout = Cout; d.R = R; d.S = S; d.stride = 1; d.pad = 0;
    const bool f16 = h->e.fp16 && (Cin % 64 == 0 || (Cin == 4 && R == 7 && S == 7));
    eng_graph_reset(h->e);
    ConvLayer& L = h->e.convs[name];
    if (L.d_w) { (void)hipFree(L.d_w); L.d_w = nullptr; }
    if (L.d_scale) { (void)hipFree(L.d_scale); L.d_scale = nullptr; }
    if (L.d_shift) { (void)hipFree(L.d_shift); L.d_shift = nullptr; }
    L.Cout = Cout; L.R = R; L.S = S; L.Cin = Cin; L.f16 = f16; L.groups = 1;
    if (f16) {
        int64_t nh = 0;
        TRY(isegmi_conv_packed_halfs(&d, &nh));
        std::vector<uint16_t> packed((size_t)nh);
        TRY(isegmi_pack_conv_weights_f16(&d, h_w_krsc, packed.data()));
        HIP_TRY(hipMalloc((void**)&L.d_w, (size_t)nh * 2));
        HIP_TRY(hipMemcpy(L.d_w, packed.data(), (size_t)nh * 2, hipMemcpyHostToDevice));
    } else {
        int64_t nf = 0;
        TRY(isegmi_conv_packed_floats(&d, &nf));
        std::vector<float> packed((size_t)nf);
        TRY(isegmi_pack_conv_weights(&d, h_w_krsc, packed.data()));
        HIP_TRY(hipMalloc((void**)&L.d_w, (size_t)nf * 4));
        HIP_TRY(hipMemcpy(L.d_w, packed.data(), (size_t)nf * 4, hipMemcpyHostToDevice));
    }
    if (h_scale) { HIP_TRY(hipMalloc((void**)&L.d_scale, (size_t)Cout * 4)); HIP_TRY(hipMemcpy(L.d_scale, h_scale, (size_t)Cout * 4, hipMemcpyHostToDevice)); }
    if (h_shift) { HIP_TRY(hipMalloc((void**)&L.d_shift, (size_t)Cout * 4)); HIP_TRY(hipMemcpy(L.d_shift, h_shift, (size_t)Cout * 4, hipMemcpyHostToDevice)); }
    if (h->e.kind == 1 && std::string(name) == kHeadCat) yolact_head_views(h->e);
    return ISEGMI_OK;
}

// a grouped 3x3 layer (ResNeXt conv2): Cin == Cout, weights [Cout][3][3][Cin / groups].  fp32 Mask R-CNN / RetinaNet engines only.
extern "C" int isegmi_engine_set_conv_grouped(isegmi_engine* h, const char* name, int Cout, int groups, const float* h_w, const float* h_scale,
                                              const float* h_shift) {
    ARG_CHECK(h && name && h_w, "null");
    ARG_CHECK(strchr(name, '[') == nullptr, "set_conv_grouped: '[' in a layer name (row-range views are the engine's)");
    ARG_CHECK(groups > 1, "set_conv_grouped: groups must be > 1 (isegmi_engine_set_conv takes the dense layers)");
    if (h->e.fp16) { set_error(std::string("grouped convolution ") + name + ": fp16 engines have no grouped kernel (fp16 ResNeXt is not built)"); return ISEGMI_ERR_ARG; }
    if (h->e.param("arch_c4", 0.0f) != 0.0f) { set_error(std::string("grouped convolution ") + name + ": the C4 body (arch_c4) has no ResNeXt form"); return ISEGMI_ERR_ARG; }
    if (h->e.kind != 2 && h->e.kind != 4) { set_error(std::string("grouped convolution ") + name + ": only the Mask R-CNN and RetinaNet engines run ResNeXt bodies"); return ISEGMI_ERR_ARG; }
    isegmi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.N = 1; d.H = 3; d.W = 3; d.Cin = Cout; d.Cout = Cout; d.R = 3; d.S = 3; d.stride = 1; d.pad = 1;
    int64_t nf = 0;
    TRY(isegmi_conv_grouped_packed_floats(&d, groups, &nf));
    std::vector<float> packed((size_t)nf);
    TRY(isegmi_pack_conv_weights_grouped(&d, groups, h_w, packed.data()));
    eng_graph_reset(h->e);
    ConvLayer& L = h->e.convs[name];
    if (L.d_w) { (void)hipFree(L.d_w); L.d_w = nullptr; }
    if (L.d_scale) { (void)hipFree(L.d_scale); L.d_scale = nullptr; }
    if (L.d_shift) { (void)hipFree(L.d_shift); L.d_shift = nullptr; }
    L.Cout = Cout; L.R = 3; L.S = 3; L.Cin = Cout; L.f16 = false; L.groups = groups;
    HIP_TRY(hipMalloc((void**)&L.d_w, (size_t)nf * 4));
    HIP_TRY(hipMemcpy(L.d_w, packed.data(), (size_t)nf * 4, hipMemcpyHostToDevice));
    if (h_scale) { HIP_TRY(hipMalloc((void**)&L.d_scale, (size_t)Cout * 4)); HIP_TRY(hipMemcpy(L.d_scale, h_scale, (size_t)Cout * 4, hipMemcpyHostToDevice)); }
    if (h_shift) { HIP_TRY(hipMalloc((void**)&L.d_shift, (size_t)Cout * 4)); HIP_TRY(hipMemcpy(L.d_shift, h_shift, (size_t)Cout * 4, hipMemcpyHostToDevice)); }
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_set_tensor(isegmi_engine* h, const char* name, const void* h_data, int64_t bytes) {
    ARG_CHECK(h && name && h_data && bytes > 0, "args");
    eng_graph_reset(h->e);
    h->e.vit_cls_rows_in = nullptr;
    RawBuf& b = h->e.tensors[name];
    if (b.d) { (void)hipFree(b.d); b.d = nullptr; }
    HIP_TRY(hipMalloc(&b.d, (size_t)bytes));
    HIP_TRY(hipMemcpy(b.d, h_data, (size_t)bytes, hipMemcpyHostToDevice));
    b.bytes = bytes;
    return ISEGMI_OK;
}

extern "C" int isegmi_yolact_forward(isegmi_engine* h, const float* d_images_nhwc3, int N) {
    ARG_CHECK(h && d_images_nhwc3, "null");
    ARG_CHECK(h->e.kind == 1, "engine is not a yolact engine");
    ARG_CHECK(N > 0 && N <= h->e.max_batch, "batch size");
    Engine& e = h->e;
    // backbone lane of this forward: consecutive forwards alternate while step_overlap is in force (an engine-side counter, whatever input slot
    // the caller reads: a resident batch is read by both lanes)
    bool two = false;
    TRY(lanes_active(e, &two));
    e.lane = two ? (e.lane_next++ & 1) : 0;
    e.last_lanes = two ? 2 : 1;
    if (e.lane == 1) { e.lane1_busy = true; ++e.lane1_forwards; }
    else if (!two && e.lane1_busy) {  // back to one lane with lane 1 still in flight (a parameter or mode switch without a sync): lane 0 follows it
        hipEvent_t ev;
        TRY(eng_next_event(e, &ev));
        HIP_TRY(hipEventRecord(ev, e.lane_stream[1]));
        HIP_TRY(hipStreamWaitEvent(e.lane_stream[0], ev, 0));
        e.lane1_busy = false;
    }
    int rc = eng_wait_upload(e, d_images_nhwc3, (int64_t)N * e.H * e.W * 3 * 4, e.lane_stream[e.lane]);
    if (rc == ISEGMI_OK) {
        char key[96];
        snprintf(key, sizeof(key), "yolact:%d:%p", N, (const void*)d_images_nhwc3);
        rc = eng_graph_run(e, key, [&]() { return yolact_forward(e, d_images_nhwc3, N); });
    }
    e.lane = 0;
    if (rc == ISEGMI_OK) { e.last_N = N; e.coeff_cols_valid = !yolact_lazy_coeffs(e, N); }   // (here, not in the graph body: a replay runs no host code)
    return rc;
}

extern "C" int isegmi_yolact_postprocess(isegmi_engine* h, int out_h, int out_w) {
    ARG_CHECK(h, "null");
    ARG_CHECK(h->e.kind == 1, "engine is not a yolact engine");
    ARG_CHECK(out_h > 0 && out_w > 0, "output size");
    return yolact_postprocess(h->e, out_h, out_w);
}

extern "C" int isegmi_yolact_postprocess_sizes(isegmi_engine* h, const int32_t* h_image_hw, int N) {
    ARG_CHECK(h && h_image_hw, "null");
    ARG_CHECK(h->e.kind == 1, "engine is not a yolact engine");
    ARG_CHECK(N == h->e.last_N, "postprocess_sizes: N must be the last forward's batch");
    int ph = 0, pw = 0;
    for (int i = 0; i < N; ++i) { ph = h_image_hw[2 * i] > ph ? h_image_hw[2 * i] : ph; pw = h_image_hw[2 * i + 1] > pw ? h_image_hw[2 * i + 1] : pw; }
    ARG_CHECK(ph > 0 && pw > 0, "image sizes");
    return yolact_postprocess(h->e, ph, pw, h_image_hw);
}

extern "C" int isegmi_engine_sync(isegmi_engine* h) {
    ARG_CHECK(h, "null");
    if (h->e.copy) HIP_TRY(hipStreamSynchronize(h->e.copy));  // an upload_async without a consumer yet: the host may reuse its pinned source after sync()
    HIP_TRY(hipStreamSynchronize(h->e.stream));
    if (h->e.lane_stream[1]) HIP_TRY(hipStreamSynchronize(h->e.lane_stream[1]));
    if (h->e.heads) HIP_TRY(hipStreamSynchronize(h->e.heads));
    if (h->e.tail) HIP_TRY(hipStreamSynchronize(h->e.tail));
    for (int l = 0; l < 2; ++l) h->e.in_pending[l] = h->e.lat_pending[l] = false;
    h->e.lane1_busy = false;
    h->e.tail_pending = false;
    h->e.heads_pending = false;
    for (auto& u : h->e.uploads) u.waited = ~0u;  // the copy stream has drained: nothing is left to wait for
    collect_times(h->e);
    return ISEGMI_OK;
}

// Asynchronous input upload: `h_src` must be pinned host memory (isegmi_malloc_host) that stays untouched until the forward
// consuming `d_dst` has been enqueued and the engine synchronised (or a later upload_async to the same d_dst returned and was
// synchronised).  The copy runs on the engine's copy stream, after the last enqueued forward has consumed ITS input (so one device
// buffer may be reused every step, two alternate without any wait).  Each destination has its own completion event and only the
// consumer of that destination (isegmi_engine_preprocess_u8 reading it, or the forward taking it as its input) waits on it: an upload
// of batch i+1 enqueued BEFORE forward i does not hold forward i back.
extern "C" int isegmi_engine_upload_async(isegmi_engine* h, void* d_dst, const void* h_src, int64_t bytes) {
    ARG_CHECK(h && d_dst && h_src && bytes > 0, "upload args");
    Engine& e = h->e;
    for (int l = 0; l < 2; ++l)   // every lane's last read of its input (the rule: eng_input_consumed)
        if (e.in_pending[l]) { HIP_TRY(hipStreamWaitEvent(e.copy, e.in_done[l], 0)); e.in_pending[l] = false; }
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, e.copy));
    return eng_note_upload(e, d_dst, bytes);
}

// Device front end (see preprocess_u8_kernel).  When its uint8 source is the destination of a pending upload_async the kernel goes to the
// COPY stream, right behind that copy: batch i+1's transform then runs under forward i instead of sitting in the main stream in front of
// it (where it would hold forward i back until upload i+1 has crossed PCIe), and the forward that takes d_out as its input waits for it
// like for an upload.  Otherwise (synchronous isegmi_h2d of the bytes) it runs on the main stream, in front of the next forward.
// (hflip: the mirrored views of TEST.BBOX_AUG, isegmi_engine_preprocess_u8_flip; the scheduling is the same)
static int engine_preprocess_u8(isegmi_engine* h, const uint8_t* d_u8, int N, int Hin, int Win, float* d_out, int Hout, int Wout, int Hpad, int Wpad,
                                int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, int hflip) {
    ARG_CHECK(h && N > 0, "preprocess args");
    Engine& e = h->e;
    const int64_t src_bytes = (int64_t)N * Hin * Win * 3, dst_bytes = (int64_t)N * out_img_stride * 4;
    bool on_copy = false;  // the source holds an upload the main stream has not been ordered behind: stay on the copy stream, behind it
    for (auto& u : e.uploads) {
        const char* p = (const char*)d_u8;
        if (!(u.waited & 1u) && p < u.dst + u.bytes && u.dst < p + src_bytes) on_copy = true;
    }
    if (on_copy) {
        // d_out's previous reader is fenced by upload_async's wait on in_done, which precedes the copy in this stream
        {
            OpScope op(e, e.copy, "front end (uint8 -> resize / normalise / pad -> fp32 input)", (double)src_bytes + (double)dst_bytes);
            TRY(preprocess_u8_launch(d_u8, N, Hin, Win, d_out, Hout, Wout, Hpad, Wpad, out_img_stride, mean3, std3, swap_rb, e.copy, hflip));
        }
        // (The source's upload entry stays UNCONSUMED: a batch is several launches over one staging buffer -- one per image of a Mask R-CNN batch --
        // and every one of them must find it and stay on the copy stream; marking it consumed here sent image 2 of a batch to the main stream,
        // ahead of its H2D copy.  A staging buffer that is re-allocated goes through sync(), which clears every entry: nothing piles up.)
        return eng_note_upload(e, d_out, dst_bytes);
    }
    TRY(eng_wait_upload(e, d_u8, src_bytes, e.stream));
    {
        OpScope op(e, e.stream, "front end (uint8 -> resize / normalise / pad -> fp32 input)", (double)src_bytes + (double)dst_bytes);
        TRY(preprocess_u8_launch(d_u8, N, Hin, Win, d_out, Hout, Wout, Hpad, Wpad, out_img_stride, mean3, std3, swap_rb, e.stream, hflip));
    }
    // two lanes: the forward that reads d_out may run on lane 1, which is not behind this (lane 0) main-stream launch -- it waits as for an upload
    if (e.lane_state == 1) return eng_note_upload(e, d_out, dst_bytes, e.stream, 1u);
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_preprocess_u8(isegmi_engine* h, const uint8_t* d_u8, int N, int Hin, int Win, float* d_out, int Hout, int Wout,
                                           int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb) {
    return engine_preprocess_u8(h, d_u8, N, Hin, Win, d_out, Hout, Wout, Hpad, Wpad, out_img_stride, mean3, std3, swap_rb, 0);
}
extern "C" int isegmi_engine_preprocess_u8_flip(isegmi_engine* h, const uint8_t* d_u8, int N, int Hin, int Win, float* d_out, int Hout, int Wout,
                                                int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, int hflip) {
    return engine_preprocess_u8(h, d_u8, N, Hin, Win, d_out, Hout, Wout, Hpad, Wpad, out_img_stride, mean3, std3, swap_rb, hflip);
}

// PIL-exact resize + normalise + pad from the ORIGINAL bytes (csrc/resample.hip), scheduled exactly as engine_preprocess_u8: the image
// table, the coefficient tables and the pixels are one blob, so one upload entry decides the stream, and nothing here synchronises.
extern "C" int isegmi_engine_resample_u8(isegmi_engine* h, const uint8_t* d_blob, int64_t blob_bytes, int64_t table_off, const int32_t* h_table, int N,
                                         int64_t coeff_off, int64_t coeff_words, int64_t src_off, float* d_out, int planes, int Hpad, int Wpad,
                                         int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, float fill) {
    ARG_CHECK(h && d_blob && h_table && d_out && N > 0 && planes > 0, "resample args");
    ARG_CHECK(table_off >= 0 && table_off % 4 == 0 && coeff_off >= 0 && coeff_off % 4 == 0 && coeff_words >= 0 && src_off >= 0 &&
              table_off + (int64_t)N * ISEGMI_RESAMPLE_ENTRY_WORDS * 4 <= blob_bytes && coeff_off + coeff_words * 4 <= blob_bytes && src_off <= blob_bytes,
              "resample blob layout (table, coefficients and pixels inside the blob; the two tables on 4-byte offsets)");
    ARG_CHECK(((uintptr_t)d_blob & 3u) == 0, "resample blob alignment");
    Engine& e = h->e;
    const int64_t dst_bytes = (int64_t)planes * out_img_stride * 4;
    bool on_copy = false;  // (the rule of engine_preprocess_u8)
    for (auto& u : e.uploads) {
        const char* p = (const char*)d_blob;
        if (!(u.waited & 1u) && p < u.dst + u.bytes && u.dst < p + blob_bytes) on_copy = true;
    }
    const int32_t* d_table = (const int32_t*)(d_blob + table_off);
    const int32_t* d_coeffs = (const int32_t*)(d_blob + coeff_off);
    const char* what = "front end (original uint8 -> PIL-exact resize / normalise / pad -> fp32 input)";
    if (on_copy) {
        {
            OpScope op(e, e.copy, what, (double)blob_bytes + (double)dst_bytes);
            TRY(resample_u8_launch(d_blob + src_off, blob_bytes - src_off, d_table, h_table, N, d_coeffs, coeff_words, d_out, planes, Hpad, Wpad,
                                   out_img_stride, mean3, std3, swap_rb, fill, nullptr, 0, e.copy));
        }
        return eng_note_upload(e, d_out, dst_bytes);
    }
    TRY(eng_wait_upload(e, d_blob, blob_bytes, e.stream));
    {
        OpScope op(e, e.stream, what, (double)blob_bytes + (double)dst_bytes);
        TRY(resample_u8_launch(d_blob + src_off, blob_bytes - src_off, d_table, h_table, N, d_coeffs, coeff_words, d_out, planes, Hpad, Wpad,
                               out_img_stride, mean3, std3, swap_rb, fill, nullptr, 0, e.stream));
    }
    if (e.lane_state == 1) return eng_note_upload(e, d_out, dst_bytes, e.stream, 1u);
    return ISEGMI_OK;
}

// Records a completion mark for the step just enqueued on the stream its results finish on; isegmi_engine_step_times returns
// the intervals between consecutive marks (ms) -- per-step latency samples of a pipelined run -- and clears them.
extern "C" int isegmi_engine_mark_step(isegmi_engine* h) {
    ARG_CHECK(h, "null");
    Engine& e = h->e;
    ARG_CHECK(e.step_marks.size() < 65536, "too many pending step marks");
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventRecord(ev, eng_results_stream(e)));
    e.step_marks.push_back(ev);
    return ISEGMI_OK;
}

// Host wait for the completion mark `back` marks before the newest one (0 = the newest): bounds how many steps a producer loop keeps in flight
// without synchronising the whole engine.
extern "C" int isegmi_engine_wait_mark(isegmi_engine* h, int back) {
    ARG_CHECK(h && back >= 0, "wait_mark args");
    Engine& e = h->e;
    if ((size_t)back >= e.step_marks.size()) return ISEGMI_OK;
    HIP_TRY(hipEventSynchronize(e.step_marks[e.step_marks.size() - 1 - (size_t)back]));
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_step_times(isegmi_engine* h, float* ms, int cap, int* count) {
    ARG_CHECK(h && ms && count && cap >= 0, "step_times args");
    Engine& e = h->e;
    int c = 0;
    if (!e.step_marks.empty()) HIP_TRY(hipEventSynchronize(e.step_marks.back()));
    for (size_t i = 1; i < e.step_marks.size() && c < cap; ++i) {
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e.step_marks[i - 1], e.step_marks[i]));
        ms[c++] = t;
    }
    for (auto& ev : e.step_marks) (void)hipEventDestroy(ev);
    e.step_marks.clear();
    *count = c;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_stream(isegmi_engine* h, void** stream) {
    ARG_CHECK(h && stream, "null");
    *stream = (void*)eng_results_stream(h->e);  // (Yolact: the tail stream)
    return ISEGMI_OK;
}

// Query a named engine buffer: device pointer, byte size, dtype (0 f32 1 i32 2 u8 3 i64), shape (up to 4 dims).
extern "C" int isegmi_engine_buffer_info(isegmi_engine* h, const char* name, void** d_ptr, int64_t* bytes, int32_t* dtype,
                                         int64_t* shape4, int32_t* ndim) {
    ARG_CHECK(h && name, "null");
    auto it = h->e.bufs.find(name);
    if (it == h->e.bufs.end()) { set_error(std::string("no such buffer: ") + name); return ISEGMI_ERR_ARG; }
    // lazy_coeffs: the last forward left headcat's coefficient columns unwritten; whoever asks for the buffer gets all of it
    if (h->e.kind == 1 && !h->e.coeff_cols_valid && it->first == "headcat") TRY(yolact_fill_coeff_columns(h->e));
    const RawBuf& b = it->second;
    if (d_ptr) *d_ptr = b.d;
    if (bytes) *bytes = b.bytes;
    if (dtype) *dtype = b.dtype;
    if (ndim) *ndim = (int32_t)b.shape.size();
    if (shape4) for (size_t i = 0; i < 4; ++i) shape4[i] = i < b.shape.size() ? b.shape[i] : 1;
    return ISEGMI_OK;
}

extern "C" int isegmi_engine_memory(isegmi_engine* h, int64_t* weight_bytes, int64_t* buffer_bytes) {
    ARG_CHECK(h, "null");
    int64_t wb = 0, bb = 0;
    for (auto& kv : h->e.convs) {
        const ConvLayer& L = kv.second;
        if (L.view) continue;
        isegmi_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.N = 1; d.H = L.R; d.W = L.S; d.Cin = L.Cin; d.Cout = L.Cout; d.R = L.R; d.S = L.S; d.stride = 1;
        int64_t n = 0;
        if (L.f16) { if (isegmi_conv_packed_halfs(&d, &n) == 0) wb += n * 2; }
        else if (isegmi_conv_packed_floats(&d, &n) == 0) wb += n * 4;
        wb += (L.d_scale ? L.Cout * 4 : 0) + (L.d_shift ? L.Cout * 4 : 0);
    }
    for (auto& kv : h->e.tensors) wb += kv.second.bytes;
    for (auto& kv : h->e.bufs) bb += kv.second.bytes;
    if (weight_bytes) *weight_bytes = wb;
    if (buffer_bytes) *buffer_bytes = bb;
    return ISEGMI_OK;
}

// Copies the stage timings of the last synchronised forward: names joined by ';' and ms values.
extern "C" int isegmi_engine_get_timings(isegmi_engine* h, char* names, int names_cap, float* ms, int ms_cap, int* count) {
    ARG_CHECK(h && names && ms && count, "null");
    std::string s;
    int c = 0;
    for (auto& kv : h->e.last_times) {
        if (c >= ms_cap) break;
        if (c) s += ";";
        s += kv.first;
        ms[c++] = kv.second;
    }
    ARG_CHECK((int)s.size() + 1 <= names_cap, "names buffer too small");
    memcpy(names, s.c_str(), s.size() + 1);
    *count = c;
    return ISEGMI_OK;
}

// Conv-kernel statistics accumulated over synchronised forwards since the last call (set_param
// "conv_timing" 1): algorithmic FLOPs (2*M*Cout*R*S*Cin, stem Cin=3), summed HIP-event time of the
// conv launches on the engine stream, and the number of launches.  Resets the accumulators.
extern "C" int isegmi_engine_conv_stats(isegmi_engine* h, double* flops, double* ms, int64_t* launches) {
    ARG_CHECK(h && flops && ms && launches, "null");
    *flops = h->e.conv_flops; *ms = h->e.conv_ms; *launches = h->e.conv_launches;
    h->e.conv_flops = 0; h->e.conv_ms = 0; h->e.conv_launches = 0;
    return ISEGMI_OK;
}

// HBM-bound stages timed under "op_timing" (call after a sync): accumulates the pending event pairs, then returns per label the summed
// HIP-event time (us), the summed ALGORITHMIC bytes and the number of timed scopes since the last call; `names` = labels joined
// by '\n'.  Resets the accumulators.
extern "C" int isegmi_engine_op_stats(isegmi_engine* h, char* names, int names_cap, double* us, double* bytes, int64_t* launches, int cap, int* count) {
    ARG_CHECK(h && names && us && bytes && launches && count && names_cap > 0 && cap > 0, "op_stats args");
    Engine& e = h->e;
    for (auto& ev : e.op_evs) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            auto& st = e.op_stats[ev.label];
            st.us += (double)ms * 1e3; st.bytes += ev.bytes; st.launches += 1;
        }
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    e.op_evs.clear();
    std::string s;
    int c = 0;
    for (auto& kv : e.op_stats) {
        if (c >= cap || (int)(s.size() + kv.first.size() + 2) > names_cap) break;
        if (c) s += "\n";
        s += kv.first;
        us[c] = kv.second.us; bytes[c] = kv.second.bytes; launches[c] = kv.second.launches;
        ++c;
    }
    memcpy(names, s.c_str(), s.size() + 1);
    *count = c;
    e.op_stats.clear();
    return ISEGMI_OK;
}

// Packs the last forward's detections into ONE contiguous record block for the all-gather:
//   [count i32 x N][box f32 x N*K*4][score f32 x N*K][class i32 x N*K][coeff f32 x N*K*32]
// (+ [proto f32 x N*PH*PW*32] when with_proto).  D2D copies on the engine stream.
extern "C" int isegmi_yolact_pack_records(isegmi_engine* h, void* d_dst, int64_t cap, int with_proto, int64_t* bytes) {
    ARG_CHECK(h && d_dst && bytes, "null");
    Engine& e = h->e;
    const int N = e.last_N;
    ARG_CHECK(N > 0, "pack before forward");
    const int K = (int)e.param("max_num_detections", 100);
    hipStream_t rs = eng_results_stream(e);
    const char* names[5] = {"det.count", "det.box", "det.score", "det.class", "det.coeff"};
    const int64_t sizes[5] = {(int64_t)N * 4, (int64_t)N * K * 16, (int64_t)N * K * 4, (int64_t)N * K * 4, (int64_t)N * K * 32 * 4};
    int64_t off = 0;
    for (int i = 0; i < 5; ++i) {
        ARG_CHECK(off + sizes[i] <= cap, "record buffer too small");
        HIP_TRY(hipMemcpyAsync((char*)d_dst + off, e.bufs[names[i]].d, (size_t)sizes[i], hipMemcpyDeviceToDevice, rs));
        off += sizes[i];
    }
    if (with_proto) {
        RawBuf& p = e.bufs["proto"];
        const int64_t pb = (int64_t)N * p.shape[1] * p.shape[2] * p.shape[3] * 4;
        ARG_CHECK(off + pb <= cap, "record buffer too small (proto)");
        HIP_TRY(hipMemcpyAsync((char*)d_dst + off, p.d, (size_t)pb, hipMemcpyDeviceToDevice, rs));
        off += pb;
    }
    if (rs == e.tail && e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));  // the copies read proto / det.*: extend the WAR fence
    *bytes = off;
    return ISEGMI_OK;
}

// Text report "label\tGFLOP\tms\tTFLOP/s" per conv layer accumulated under conv_timing; clears it.
extern "C" int isegmi_engine_conv_report(isegmi_engine* h, char* buf, int cap) {
    ARG_CHECK(h && buf && cap > 0, "args");
    std::string s;
    for (auto& kv : h->e.conv_layers) {
        char line[256];
        snprintf(line, sizeof(line), "%s\t%.3f\t%.4f\t%.2f\n", kv.first.c_str(), kv.second.first / 1e9, kv.second.second,
                 kv.second.second > 0 ? kv.second.first / (kv.second.second * 1e-3) / 1e12 : 0.0);
        s += line;
    }
    h->e.conv_layers.clear();
    ARG_CHECK((int)s.size() + 1 <= cap, "report buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return ISEGMI_OK;
}
