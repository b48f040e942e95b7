// resnet.cpp -- the ResNet trunk, once: the stem and one stage of bottleneck blocks, as the Yolact and Mask R-CNN backbones, the C4 RoI head
// and Pose2Seg (backbone and SegModule) run them.  What differs between those is data (ResStage in engine.h), not code.
#include "engine.h"

namespace isegmi {

bool eng_has_gn(Engine& e, const std::string& layer) { return e.tensors.count(layer + ".gn.weight") != 0; }

int eng_gn(Engine& e, const std::string& layer, Tensor* x, const Tensor* residual, bool relu) {
    if (e.fp16 || x->dt || (residual && residual->dt)) { set_error("GroupNorm layers run in fp32 only (" + layer + ")"); return ISEGMI_ERR_STATE; }
    auto wi = e.tensors.find(layer + ".gn.weight"), bi = e.tensors.find(layer + ".gn.bias");
    if (wi == e.tensors.end() || bi == e.tensors.end()) { set_error("GroupNorm affine not set: " + layer + ".gn.weight / .gn.bias"); return ISEGMI_ERR_STATE; }
    if (wi->second.bytes != (int64_t)x->C * 4 || bi->second.bytes != (int64_t)x->C * 4) { set_error("GroupNorm affine of " + layer + " has the wrong size"); return ISEGMI_ERR_STATE; }
    const int per = (int)e.param("gn_dim_per_gp", -1.0f);
    const int groups = per > 0 ? x->C / per : (int)e.param("gn_num_groups", 32.0f);
    if (groups <= 0 || x->C % groups || (per > 0 && x->C % per)) { set_error("GroupNorm of " + layer + ": the groups do not divide its channels"); return ISEGMI_ERR_ARG; }
    if (residual && (residual->N != x->N || residual->H != x->H || residual->W != x->W || residual->C != x->C)) { set_error("GroupNorm of " + layer + ": residual shape"); return ISEGMI_ERR_ARG; }
    void* ws = nullptr;
    const int64_t ws_bytes = groupnorm_workspace_bytes(x->N, x->H, x->W, x->C, groups);
    if (ws_bytes) TRY(eng_buf(e, "gn.ws:" + layer, ws_bytes, &ws, 2));   // one per layer: GroupNorm launches of independent branches run on different streams
    // algorithmic bytes: x once (slabs) or twice (statistics pass + apply pass), the residual once, y once
    OpScope op(e, e.cur, groupnorm_is_slab(x->H, x->W) ? "group_norm (slab: one pass)" : "group_norm (plane: statistics + apply)",
               (double)x->numel() * 4 * ((groupnorm_is_slab(x->H, x->W) ? 2 : 3) + (residual ? 1 : 0)));
    return groupnorm_launch(x->d, x->N, x->H, x->W, x->C, groups, (const float*)wi->second.d, (const float*)bi->second.d, e.param("gn_epsilon", 1e-5f),
                            residual ? residual->d : nullptr, relu ? 1 : 0, x->d, ws, ws_bytes, e.cur);
}

int resnet_stem(Engine& e, const std::string& layer, const float* d_images, int N, int H, int W, Tensor* pool) {
    const int dt = e.fp16 ? 1 : 0;
    if (eng_has_gn(e, layer)) {   // StemWithGN: conv -> GN -> ReLU -> max-pool
        Tensor x4, s;
        if (dt) { set_error("GroupNorm layers run in fp32 only (" + layer + ")"); return ISEGMI_ERR_STATE; }
        TRY(eng_act(e, "input4", N, H, W, 4, &x4));
        TRY(pad_c3_c4_launch(d_images, (int64_t)N * H * W, x4.d, e.cur));
        TRY(eng_input_consumed(e));
        TRY(eng_conv(e, layer, x4, 2, 3, 0, nullptr, "stem", &s));
        TRY(eng_gn(e, layer, &s, nullptr, true));
        TRY(eng_act(e, "pool", N, (s.H + 2 - 3) / 2 + 1, (s.W + 2 - 3) / 2 + 1, s.C, pool, 0));
        return maxpool_launch(s.d, N, s.H, s.W, s.C, 3, 2, 1, pool->d, e.cur);
    }
    Tensor x4, s;
    bool stem_fused = false;
    if (dt) {  // fp16: images are rounded to fp16 into a zero-haloed 4-channel buffer the stem kernel reads without bounds tests
        TRY(eng_act(e, "input4h", N, H + 6, (W + 7) & ~1, 4, &x4, 1));
        TRY(pad_c3_to_f16_halo_launch(d_images, N, H, W, x4.d, e.cur));
        TRY(eng_input_consumed(e));
        TRY(eng_stem_pool_f16(e, layer, x4, H, W, "pool", pool, &stem_fused));   // conv + BN + ReLU + max-pool in one launch
        if (!stem_fused) TRY(eng_conv_stem_f16(e, layer, x4, H, W, "stem", &s));
    } else {
        TRY(eng_act(e, "input4", N, H, W, 4, &x4));
        TRY(pad_c3_c4_launch(d_images, (int64_t)N * H * W, x4.d, e.cur));
        TRY(eng_input_consumed(e));
        TRY(eng_conv(e, layer, x4, 2, 3, 1, nullptr, "stem", &s));
    }
    if (!stem_fused) {
        const int Ho = (s.H + 2 - 3) / 2 + 1, Wo = (s.W + 2 - 3) / 2 + 1;
        TRY(eng_act(e, "pool", N, Ho, Wo, s.C, pool, dt));
        if (dt) TRY(maxpool_to_f16_launch(s.d, 1, N, s.H, s.W, s.C, 3, 2, 1, pool->d, e.cur));
        else TRY(maxpool_launch(s.d, N, s.H, s.W, s.C, 3, 2, 1, pool->d, e.cur));
    }
    return ISEGMI_OK;
}

// conv2 of a block as a deformable 3x3 (YOLACT++ backbones: DCNv2; the dcn/ R-CNN models: DCNv1 or DCNv2, told apart by the offset layer's 18 or 27
// channels): offsets (+ mask logits) from a plain 3x3, then the deformable conv proper over the layer's 1x1 / 9*C weights (KRSC order, bias folded into
// BN).  "dcn_fused" 1: ONE launch that samples into the MFMA operand tile (csrc/deform_conv.hip), no column buffer; 0: the nine taps sampled into
// columns -> a 1x1 over 9*C channels.  The two forms agree bit for bit.  The default is 0 in every engine and at every stage: at 800 x 1344 the fused
// launch measures 1.3-2.3 x the time of the two launches it replaces (tools/deform_conv_bench.py), so it stays opt-in.
static int dcn_conv2(Engine& e, const std::string& nm, const std::string& blk, const Tensor& t1, int stride, const std::string& out_name, Tensor* t2) {
    if (t1.dt) { set_error("the deformable-convolution backbones run in fp32 only (" + nm + ".conv2)"); return ISEGMI_ERR_STATE; }
    Tensor om, col;
    TRY(eng_conv(e, nm + ".conv2.conv_offset_mask", t1, stride, 1, 0, nullptr, blk + ".om", &om));
    if (om.C != 27 && om.C != 18) {
        set_error("deformable conv " + nm + ".conv2.conv_offset_mask has " + std::to_string(om.C) + " output channels: 27 (modulated) or 18 (offsets only)");
        return ISEGMI_ERR_ARG;
    }
    const int modulated = om.C == 27 ? 1 : 0;
    const bool fused = e.param("dcn_fused", 0.0f) != 0.0f;
    if (!fused) {
        TRY(eng_act(e, blk + ".col", t1.N, om.H, om.W, 9 * t1.C, &col));
        TRY(deform_im2col_launch((const float*)t1.d, t1.N, t1.H, t1.W, t1.C, (const float*)om.d, 3, 3, stride, 1, 1, modulated, (float*)col.d, e.cur));
        return eng_conv(e, nm + ".conv2", col, 1, 0, 1, nullptr, out_name, t2);
    }
    const auto it = e.convs.find(nm + ".conv2");
    if (it == e.convs.end()) { set_error("conv layer not set: " + nm + ".conv2"); return ISEGMI_ERR_STATE; }
    const ConvLayer& L = it->second;
    if (L.f16 || L.groups != 1 || L.R != 1 || L.S != 1 || L.Cin != 9 * t1.C) {
        set_error("deformable conv " + nm + ".conv2: the weights must be the fp32 1x1 layer over 9 * " + std::to_string(t1.C) + " channels");
        return ISEGMI_ERR_ARG;
    }
    TRY(eng_act(e, out_name, t1.N, om.H, om.W, L.Cout, t2));
    const int M = t1.N * om.H * om.W;
    ConvScope cs(e);
    cs.trace(nm + ".conv2", " (deform fused)", t1.N, t1.H, t1.W, t1.C, L.Cout, 3, stride, M, false);
    TRY(deform_conv2d_launch((const float*)t1.d, t1.N, t1.H, t1.W, t1.C, (const float*)om.d, om.C, modulated, stride, L.d_w, L.Cout, L.d_scale, L.d_shift,
                             nullptr, 1, (float*)t2->d, e.cur));
    cs.done(2.0 * M * 9.0 * t1.C * L.Cout, "%s (deform fused) [M=%d K=%d Cout=%d 3x3/%d]", (nm + ".conv2").c_str(), M, 9 * t1.C, L.Cout, stride);
    return ISEGMI_OK;
}

int resnet_stage(Engine& e, const ResStage& s, const Tensor& in, Tensor* out) {
    // Buffers by LIVENESS, not by layer (round 3): a full stage owns one t1, one t2, two alternating block outputs and its final output
    // <stage>.C.  Everything runs in order on the main stream (the shortcut of block 0 is joined before conv3), so a buffer's last reader
    // is always enqueued before its next writer.  Besides the memory (R101 bs=8: 33 x 3 buffers -> 4 x 5), a dead activation is now
    // overwritten while its lines still sit in the Infinity Cache instead of being written back to HBM behind the live traffic.
    // (The stage's final output is on its own: Yolact's C3-C5 are read by the lateral convs of the pipelined heads phase, and `before_out` guards
    // exactly those.)
    const bool alias = s.full && e.param("alias_buffers", 1.0f) != 0.0f;  // 0: one buffer per layer output (rounds 1-2; kept for A/B)
    const bool groups = e.param("conv_groups", 1.0f) != 0.0f && e.param("conv_tile", 0) == 0.0f;
    Tensor x = in;
    for (int b = 0; b < s.blocks; ++b) {
        const std::string nm = s.layers + "." + std::to_string(b), blk = s.bufs + "." + std::to_string(b);
        const std::string sg = alias ? s.stage : blk;
        const std::string out_name = !alias ? blk + ".out" : b == s.blocks - 1 ? sg + ".C" : sg + (b & 1 ? ".outB" : ".outA");
        const int st = b == 0 ? s.stride : 1, st1 = s.stride_in_1x1 ? st : 1, st2 = s.stride_in_1x1 ? 1 : st;
        const bool proj = s.proj_by_name ? e.convs.count(nm + ".downsample.0") != 0 : b == 0;
        // BottleneckWithGN: conv1-GN-ReLU, conv2-GN-ReLU, conv3-GN + identity, ReLU (the projection is followed by its own GN).  Each convolution runs
        // bare (no activation, no residual); the GroupNorm launch behind it carries the ReLU, and conv3's the residual add too.
        const bool gn = eng_has_gn(e, nm + ".conv1");
        const int act = gn ? 0 : 1;
        // the previous user of the stage's output buffer must have read it: one wait, ahead of whichever launch writes it (they are the first
        // thing of the phase that reads it, so this wait practically never blocks)
        bool fence = b == s.blocks - 1 && s.before_out != nullptr;
        Tensor idt = x, t1, t2, y;
        if (s.full && x.dt == 1 && (b > 0 || st == 1)) {
            // fp16: the identity blocks of res2 / res3 and res2's first block (projection included) are ONE launch each, t1 / t2 stay in LDS
            // (csrc/bottleneck_f16.hip); the alternating outA / outB are what keeps that launch from running in place
            if (fence) { HIP_TRY(hipStreamWaitEvent(e.stream, s.before_out, 0)); fence = false; }
            bool fused = false;
            TRY(eng_bottleneck_f16(e, nm, x, b == 0, out_name, &y, &fused));
            if (fused) { x = y; continue; }
        }
        const bool pair = s.full && proj && x.dt == 0 && groups;
        if (pair) {  // fp32: the projection shortcut and conv1 read the same x: one grouped launch (round 5) instead of a side stream
            std::vector<ConvGroupItem> g(2);
            g[0].layer = nm + ".conv1"; g[0].in = x; g[0].stride = st1; g[0].act = act; g[0].out_name = sg + ".t1"; g[0].out = &t1;
            g[1].layer = nm + ".downsample.0"; g[1].in = x; g[1].stride = st; g[1].out_name = blk + ".ds"; g[1].out = &idt;
            TRY(eng_conv_group(e, g));
            if (gn) {
                TRY(eng_gn(e, nm + ".conv1", &t1, nullptr, true));
                TRY(eng_gn(e, nm + ".downsample.0", &idt, nullptr, false));
            }
        } else {
            if (proj && s.full) {  // the projection shortcut is independent of conv1 -> conv2: side stream
                TRY(eng_fork(e, 0));
                SideScope sc(e, 0);
                TRY(eng_conv(e, nm + ".downsample.0", x, st, 0, 0, nullptr, blk + ".ds", &idt));
                if (gn) TRY(eng_gn(e, nm + ".downsample.0", &idt, nullptr, false));
            } else if (proj) {
                TRY(eng_conv(e, nm + ".downsample.0", x, st, 0, 0, nullptr, blk + ".ds", &idt));
                if (gn) TRY(eng_gn(e, nm + ".downsample.0", &idt, nullptr, false));
            }
            TRY(eng_conv(e, nm + ".conv1", x, st1, 0, act, nullptr, sg + ".t1", &t1, false, /*may_split=*/s.full && b > 0));   // (`conv_split_k`: see eng_conv)
            if (gn) TRY(eng_gn(e, nm + ".conv1", &t1, nullptr, true));
        }
        // ResNeXt: conv2 uploaded with grouped weights (isegmi_engine_set_conv_grouped) runs the grouped kernel through eng_conv like any other layer; t1 /
        // t2 take their width from the weights, in the full and in the plain form.  Built next to FrozenBN and in fp32 only.
        const auto c2 = e.convs.find(nm + ".conv2");
        if (c2 != e.convs.end() && c2->second.groups > 1) {
            if (gn) { set_error("grouped convolution " + nm + ".conv2 with GroupNorm weights: ResNeXt bodies with GroupNorm are not built"); return ISEGMI_ERR_STATE; }
            if (t1.dt) { set_error("grouped convolution " + nm + ".conv2 in an fp16 engine: fp16 ResNeXt is not built"); return ISEGMI_ERR_STATE; }
        }
        if (gn && e.convs.count(nm + ".conv2.conv_offset_mask")) { set_error("deformable conv " + nm + ".conv2 with GroupNorm weights: DCN bodies with GroupNorm are not built"); return ISEGMI_ERR_STATE; }
        if (e.convs.count(nm + ".conv2.conv_offset_mask")) TRY(dcn_conv2(e, nm, blk, t1, st2, sg + ".t2", &t2));
        else TRY(eng_conv(e, nm + ".conv2", t1, st2, 1, act, nullptr, sg + ".t2", &t2, false, /*may_split=*/s.full));
        if (gn) TRY(eng_gn(e, nm + ".conv2", &t2, nullptr, true));
        if (proj && s.full && !pair) TRY(eng_join(e, 0));
        if (fence) HIP_TRY(hipStreamWaitEvent(e.stream, s.before_out, 0));
        TRY(eng_conv(e, nm + ".conv3", t2, 1, 0, act, gn ? nullptr : &idt, out_name, &y, false, /*may_split=*/s.full));
        if (gn) TRY(eng_gn(e, nm + ".conv3", &y, &idt, true));
        x = y;
    }
    *out = x;
    return ISEGMI_OK;
}

}  // namespace isegmi
