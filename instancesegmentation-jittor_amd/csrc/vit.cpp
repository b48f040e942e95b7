// vit.cpp -- the ViT classifier engine (model_kind 7; [UPSTREAM-RECALL] Dosovitskiy et al. in the PyTorch / timm layout, unverified:
// the reference's ViT.jittor directory is empty).  fp32, pre-LN blocks, a learned class token and position embedding, the head on the class token:
//
//   patchify (csrc/vit_ops.hip) -> patch_embed.proj as a 1x1 convolution over P * P * 3 channels, written straight into rows 1 .. T-1 of vit.tokens with the
//   position embedding of those rows as its residual (vit.pos_rows: pos_embed[1:] tiled over max_batch by the host); row 0 of every image is the constant
//   vit.cls_row = cls_token + pos_embed[0], copied in when the buffer or the tensors are new.
//   depth times:  x1 = x + proj(attention(qkv(LN1(x))));  x = x1 + fc2(GELU(fc1(LN2(x1))))      (vit.x1 / vit.x2; block 0 reads vit.tokens)
//   cls.logits = head(LN(x)[:, 0]) -> cls.prob (softmax) -> cls.topk_val / cls.topk_idx (the vit_topk largest probabilities, isegmi_op_topk's order)
//
// Every linear layer is a 1x1 fp32 MFMA convolution over tokens (bias as shift, the residual in the epilogue) and is counted in conv_stats; vit.ln, vit.qkv,
// vit.attn and vit.mlp hold the last block's tensors.  Everything runs on the engine's main stream.  fp16 and graph are refused.
#include "engine.h"

namespace isegmi {

static int vit_tensor(Engine& e, const std::string& name, int64_t floats, const float** out) {
    auto it = e.tensors.find(name);
    if (it == e.tensors.end()) { set_error("vit: tensor not set: " + name); return ISEGMI_ERR_STATE; }
    if (it->second.bytes != floats * 4) { set_error("vit: tensor " + name + " has " + std::to_string(it->second.bytes / 4) + " floats, expected " + std::to_string(floats)); return ISEGMI_ERR_STATE; }
    *out = (const float*)it->second.d;
    return ISEGMI_OK;
}

static int vit_ln(Engine& e, const std::string& norm, const float* x, int64_t rows, int D, int64_t x_stride, float eps, float* out) {
    const float *ga, *be;
    TRY(vit_tensor(e, norm + ".weight", D, &ga));
    TRY(vit_tensor(e, norm + ".bias", D, &be));
    OpScope op(e, e.stream, "layer_norm", 2.0 * (double)rows * D * 4);
    return vit_layer_norm_launch(x, rows, D, x_stride, ga, be, eps, out, D, e.stream);
}

struct VitShape { int D, depth, heads, mlp, P, ncls, topk, gelu_tanh, gh, gw, T; float eps; };

static int vit_shape(Engine& e, VitShape* s) {
    s->D = (int)e.param("vit_dim", 0.0f); s->depth = (int)e.param("vit_depth", 0.0f); s->heads = (int)e.param("vit_heads", 0.0f);
    s->mlp = (int)e.param("vit_mlp_dim", 0.0f); s->P = (int)e.param("vit_patch", 0.0f); s->ncls = (int)e.param("vit_num_classes", 0.0f);
    s->topk = (int)e.param("vit_topk", 5.0f); s->eps = e.param("vit_ln_eps", 1e-6f);
    const float gt = e.param("vit_gelu_tanh", 0.0f);
    s->gelu_tanh = gt != 0.0f ? 1 : 0;
    if (gt != 0.0f && gt != 1.0f) { set_error("vit: vit_gelu_tanh must be 0 (erf) or 1 (tanh)"); return ISEGMI_ERR_ARG; }
    if (s->heads < 1 || s->D != 64 * s->heads) { set_error("vit: vit_dim must be 64 * vit_heads (head dimension 64 only)"); return ISEGMI_ERR_ARG; }
    if (s->depth < 1) { set_error("vit: vit_depth must be at least 1"); return ISEGMI_ERR_ARG; }
    if (s->mlp < 32 || s->mlp % 32) { set_error("vit: vit_mlp_dim must be a positive multiple of 32"); return ISEGMI_ERR_ARG; }
    if (s->P != 16 && s->P != 32) { set_error("vit: vit_patch must be 16 or 32 (3 * P * P a multiple of 32)"); return ISEGMI_ERR_ARG; }
    if (e.H % s->P || e.W % s->P) { set_error("vit: the canvas sides must be multiples of vit_patch"); return ISEGMI_ERR_ARG; }
    if (s->ncls < 2 || s->ncls > 8192) { set_error("vit: vit_num_classes must be 2..8192"); return ISEGMI_ERR_ARG; }
    if (s->topk < 1 || s->topk > 64) { set_error("vit: vit_topk must be 1..64"); return ISEGMI_ERR_ARG; }
    if (!(s->eps >= 0.0f)) { set_error("vit: vit_ln_eps must be a non-negative number"); return ISEGMI_ERR_ARG; }
    s->gh = e.H / s->P; s->gw = e.W / s->P; s->T = s->gh * s->gw + 1;
    if (s->T > 1024) { set_error("vit: more than 1024 tokens (T = H / P * W / P + 1)"); return ISEGMI_ERR_ARG; }
    return ISEGMI_OK;
}

static int vit_forward(Engine& e, const VitShape& s, const float* d_images, int N) {
    e.cur = e.stream;
    hipStream_t st = e.stream;
    const int D = s.D, T = s.T, G = s.gh * s.gw;
    const int64_t B = e.max_batch;
    eng_mark(e, "start");

    // ---- embedding
    Tensor patches;
    TRY(eng_act(e, "vit.patches", N, s.gh, s.gw, s.P * s.P * 3, &patches));
    {
        OpScope op(e, st, "patchify", 2.0 * (double)patches.numel() * 4);
        TRY(vit_patchify_launch(d_images, N, e.H, e.W, s.P, patches.d, st));
    }
    TRY(eng_input_consumed(e));
    void* q;
    TRY(eng_buf(e, "vit.tokens", B * T * D * 4, &q, 0, {N, T, D}));
    float* tokens = (float*)q;
    const float *cls_row, *pos_rows;
    TRY(vit_tensor(e, "vit.cls_row", D, &cls_row));
    TRY(vit_tensor(e, "vit.pos_rows", B * G * D, &pos_rows));
    if (e.vit_cls_rows_in != (const void*)tokens) {
        for (int64_t n = 0; n < B; ++n) HIP_TRY(hipMemcpyAsync(tokens + n * T * D, cls_row, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        e.vit_cls_rows_in = tokens;
    }
    TRY(eng_conv_into(e, "patch_embed.proj", patches, 1, 0, 0, tokens + D, G, (int64_t)T * D, D, false, pos_rows));
    eng_mark(e, "embed");

    // ---- blocks
    Tensor x;
    x.d = tokens; x.N = N; x.H = T; x.W = 1; x.C = D;
    Tensor ln, qkv, attn, x1, h1, x2;
    TRY(eng_act(e, "vit.ln", N, T, 1, D, &ln));
    TRY(eng_act(e, "vit.attn", N, T, 1, D, &attn));
    for (int i = 0; i < s.depth; ++i) {
        const std::string b = "blocks." + std::to_string(i);
        TRY(vit_ln(e, b + ".norm1", x.d, (int64_t)N * T, D, D, s.eps, ln.d));
        TRY(eng_conv(e, b + ".attn.qkv", ln, 1, 0, 0, nullptr, "vit.qkv", &qkv));
        if (qkv.C != 3 * D) { set_error("vit: " + b + ".attn.qkv must have 3 * vit_dim output channels"); return ISEGMI_ERR_STATE; }
        {   // algorithmic bytes: qkv once, the output once
            OpScope op(e, st, "attention (softmax(q k^T / 8) v, all heads)", 4.0 * (double)N * T * D * 4);
            TRY(vit_attention_launch(qkv.d, N, T, s.heads, attn.d, st));
        }
        TRY(eng_conv(e, b + ".attn.proj", attn, 1, 0, 0, &x, "vit.x1", &x1));
        TRY(vit_ln(e, b + ".norm2", x1.d, (int64_t)N * T, D, D, s.eps, ln.d));
        TRY(eng_conv(e, b + ".mlp.fc1", ln, 1, 0, 0, nullptr, "vit.mlp", &h1));
        {
            OpScope op(e, st, "gelu", 2.0 * (double)h1.numel() * 4);
            TRY(vit_gelu_launch(h1.d, h1.d, h1.numel(), s.gelu_tanh, st));
        }
        TRY(eng_conv(e, b + ".mlp.fc2", h1, 1, 0, 0, &x1, "vit.x2", &x2));
        if (x1.C != D || x2.C != D) { set_error("vit: " + b + ": attn.proj and mlp.fc2 must have vit_dim output channels"); return ISEGMI_ERR_STATE; }
        x = x2;
    }
    eng_mark(e, "blocks");

    // ---- head: the final norm on the class-token rows only
    Tensor cn;
    TRY(eng_act(e, "vit.cls_norm", N, 1, 1, D, &cn));
    TRY(vit_ln(e, "norm", x.d, N, D, (int64_t)T * D, s.eps, cn.d));
    float *logits, *prob, *tv; int32_t *ti, *tc;
    TRY(eng_buf(e, "cls.logits", B * s.ncls * 4, &q, 0, {N, s.ncls})); logits = (float*)q;
    TRY(eng_buf(e, "cls.prob", B * s.ncls * 4, &q, 0, {N, s.ncls})); prob = (float*)q;
    TRY(eng_buf(e, "cls.topk_val", B * s.topk * 4, &q, 0, {N, s.topk})); tv = (float*)q;
    TRY(eng_buf(e, "cls.topk_idx", B * s.topk * 4, &q, 1, {N, s.topk})); ti = (int32_t*)q;
    TRY(eng_buf(e, "cls.topk_cnt", B * 4, &q, 1, {N})); tc = (int32_t*)q;
    {
        auto it = e.convs.find("head");
        if (it != e.convs.end() && it->second.Cout != s.ncls) { set_error("vit: head must have vit_num_classes output channels"); return ISEGMI_ERR_STATE; }
    }
    TRY(eng_conv_into(e, "head", cn, 1, 0, 0, logits, 1, s.ncls, s.ncls));
    {
        OpScope op(e, st, "class softmax + top-k", 3.0 * (double)N * s.ncls * 4);
        TRY(vit_softmax_launch(logits, N, s.ncls, prob, st));
        TRY(topk_launch(prob, s.ncls, N, s.ncls, s.topk, nullptr, 1, tv, ti, tc, st));
    }
    eng_mark(e, "head");
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_vit_forward(isegmi_engine* h, const float* d_images, int N) {
    ARG_CHECK(h && d_images, "null");
    Engine& e = h->e;
    ARG_CHECK(e.kind == 7, "engine is not a ViT engine");
    ARG_CHECK(N > 0 && N <= e.max_batch, "batch size");
    if (e.param("fp16", 0.0f) != 0.0f || e.fp16) { set_error("vit: fp16 is not supported (fp32 only)"); return ISEGMI_ERR_ARG; }
    if (e.param("graph", 0.0f) != 0.0f) { set_error("vit: graph capture is not supported (graph must be 0)"); return ISEGMI_ERR_ARG; }
    VitShape s;
    TRY(vit_shape(e, &s));
    TRY(eng_wait_upload(e, d_images, (int64_t)N * e.H * e.W * 3 * 4, e.stream));
    const int rc = vit_forward(e, s, d_images, N);
    e.cur = e.stream;
    if (rc == ISEGMI_OK) e.last_N = N;
    return rc;
}
