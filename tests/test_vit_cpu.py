"""The ViT restatements of tests/vit_ref.py against float64, the configuration refusals, the patch-embedding weight order and the command line.
Nothing here needs a GPU.  u = 2^-24 throughout; every bound below is derived from the rounding count of the fp32 sequence it bounds, except the
whole-model one, which has no tractable derivation and is set by torch's own fp32 operators (four times their error, as DESIGN.md 18 records)."""
import math

import numpy as np
import pytest

import vit_ref as vr
from vit_ref import erf_sweep

U, TINY = vr.U, vr.TINY


def test_dm_erf_against_math_erf():
    """|x| <= 1: x * T(x^2), a degree-6 Horner form with 12 roundings over terms of magnitude sum |c_i| z^i <= 1.65 against |T| >= 0.84, x^2 and the last
    product 2 more, Cephes' approximation error below 3u: relative error below (12 * 2 + 5 + 3) u = 32 u (one subnormal ulp added for tiny x).
    |x| > 1: erfc = exp(-x^2) / x * P(1 / x^2): 16 Horner roundings over sum |P_i| / |P| <= 8 -> 128 u, exp's argument x^2 u (x^2 <= 4 where erfc matters)
    and exp / division / products 8 u more: relative 140 u of erfc(1) = 0.157 at most, i.e. 22 u absolute; for x >= 2 the R form (ratio 1.4) times erfc(2) =
    0.005 is far below.  1 - erfc adds u / 2.  Absolute error below 32 u."""
    x = erf_sweep()
    got = vr.dm_erf(x).astype(np.float64)
    want = np.asarray([math.erf(float(v)) for v in x])
    err = np.abs(got - want)
    small = np.abs(x) <= 1
    normal = small & (np.abs(want) > 1e-30)
    print("dm_erf: max relative error (1e-30 < |x| <= 1) %.3g u, max absolute error (|x| > 1) %.3g u" %
          ((err[normal] / np.abs(want[normal])).max() / U, err[~small].max() / U))
    assert (err[small] <= 32 * U * np.abs(want[small]) + TINY).all()
    assert (err[~small] <= 32 * U).all()
    assert np.array_equal(np.signbit(got), np.signbit(x.astype(np.float64)))        # odd, -0 -> -0
    assert vr.dm_erf(np.float32([30.0, -30.0, 1e10])).tolist() == [1.0, -1.0, 1.0]
    assert np.isnan(vr.dm_erf(np.float32([np.nan]))[0])


@pytest.mark.parametrize("gelu_tanh", [False, True])
def test_gelu_against_float64(gelu_tanh):
    """y = (x / 2) (1 + t).  erf form: t carries dm_erf's 32 u plus the argument's two roundings through erf' (|t erf'(t)| <= 0.5: 1 u): 34 u absolute.
    tanh form: the argument has 5 roundings, |a tanh'(a)| <= 0.45 -> 2.3 u; dm_tanh itself (exp 2 u, the quotient 4 u of at most 0.45, the subtraction)
    below 8 u: 11 u.  Then 1 + t, x / 2 (exact) and the product: 3 u relative."""
    import torch
    x = np.concatenate([erf_sweep(), np.linspace(-12, 12, 2001).astype(np.float32)])
    x = x[np.abs(x) < 1e18]      # x^3 stays finite in the tanh form
    got = vr.gelu(x, gelu_tanh).astype(np.float64)
    want = torch.nn.functional.gelu(torch.from_numpy(x.astype(np.float64)), approximate="tanh" if gelu_tanh else "none").numpy()
    bound = np.abs(x.astype(np.float64)) / 2 * (11 if gelu_tanh else 34) * U + 3 * U * np.abs(want) + TINY
    err = np.abs(got - want)
    print("gelu(tanh=%d): max error / bound %.3f" % (gelu_tanh, (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("D", [4, 8, 32, 192, 252, 256, 260, 768, 1024, 1280, 2044, 2048])
def test_layer_norm_against_float64(D):
    """The bound is vit_ref.ln_bound (shared with the GPU tests).  D = 4 and 8: one and two live lanes; 252 / 256 / 260: one slot either side of 64 slots;
    1280: ViT-H; 2044 / 2048: the last partial and the last full set of 8 slots per lane."""
    rng = np.random.default_rng(D)
    x = rng.standard_normal((7, D)).astype(np.float32)
    x[1] += 1000.0                       # |mean| >> sigma: the shifted sums keep their digits
    x[2] = x[2] * 1e-3 + 5.0
    ga = rng.uniform(0.5, 1.5, D).astype(np.float32); be = (rng.standard_normal(D) * 0.1).astype(np.float32)
    got = vr.layer_norm(x, ga, be, 1e-6).astype(np.float64)
    want = vr.layer_norm_float64(x, ga, be, 1e-6)
    err, bound = np.abs(got - want), vr.ln_bound(x, ga, be, 1e-6)
    print("layer_norm D=%d: max error / bound %.3f" % (D, (err / bound).max()))
    assert (err <= bound).all()
    const = np.full((1, D), 3.25, np.float32)     # a constant row: variance exactly 0, y = beta
    assert np.array_equal(vr.layer_norm(const, ga, be, 1e-6), be[None])


@pytest.mark.parametrize("T", [1, 17, 197, 576, 577, 1024])
def test_attention_against_float64(T):
    """The bound and its derivation are vit_ref.attention_bound (shared with the GPU tests).  576 / 577: either side of the kernel's 4 -> 2 wavefront fork;
    1024: its maximum."""
    rng = np.random.default_rng(T)
    heads = 2
    qkv = rng.standard_normal((1, T, 3 * heads * 64)).astype(np.float32)
    got = vr.attention(qkv, heads).astype(np.float64)
    want, bound = vr.attention_bound(qkv, heads)
    err = np.abs(got - want)
    print("attention T=%d: max error / bound %.4f" % (T, (err / bound).max()))
    assert (err <= bound).all()
    if T == 1:
        assert np.array_equal(vr.attention(qkv, heads), qkv[:, :, 2 * heads * 64:])      # one key: p = 1, o = v


def tiny_cfg(**kw):
    from isegmi.vit import ViTConfig
    return ViTConfig(**dict(dict(dim=128, depth=2, heads=2, mlp_dim=256, patch=16, num_classes=10, topk=3), **kw))


def torch_forward(sd, cfg, images, dtype):
    import torch
    Fn = torch.nn.functional
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    x = torch.from_numpy(images).to(dtype).permute(0, 3, 1, 2)
    x = Fn.conv2d(x, t["patch_embed.proj.weight"], t["patch_embed.proj.bias"], stride=cfg.patch).flatten(2).transpose(1, 2)
    x = torch.cat([t["cls_token"].expand(x.shape[0], -1, -1), x], 1) + t["pos_embed"]
    N, T, D = x.shape
    for i in range(cfg.depth):
        b = "blocks.%d." % i
        h = Fn.layer_norm(x, (D,), t[b + "norm1.weight"], t[b + "norm1.bias"], cfg.ln_eps)
        qkv = Fn.linear(h, t[b + "attn.qkv.weight"], t[b + "attn.qkv.bias"]).reshape(N, T, 3, cfg.heads, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / 8, -1) @ qkv[2]
        x = x + Fn.linear(a.transpose(1, 2).reshape(N, T, D), t[b + "attn.proj.weight"], t[b + "attn.proj.bias"])
        h = Fn.layer_norm(x, (D,), t[b + "norm2.weight"], t[b + "norm2.bias"], cfg.ln_eps)
        h = Fn.gelu(Fn.linear(h, t[b + "mlp.fc1.weight"], t[b + "mlp.fc1.bias"]), approximate="tanh" if cfg.gelu_tanh else "none")
        x = x + Fn.linear(h, t[b + "mlp.fc2.weight"], t[b + "mlp.fc2.bias"])
    x = Fn.layer_norm(x, (D,), t["norm.weight"], t["norm.bias"], cfg.ln_eps)
    return Fn.linear(x[:, 0], t["head.weight"], t["head.bias"]).numpy()


@pytest.mark.parametrize("gelu_tanh", [False, True])
def test_tiny_model_against_torch_float64(gelu_tanh):
    """The composed forward against the same model built from torch.nn.functional in float64.  No derivation through two blocks is tractable, so the
    bound is the documented fallback: torch's own fp32 operators against float64 on the same inputs, times four (the summation orders differ)."""
    from isegmi.weights import vit_random_state_dict
    cfg = tiny_cfg(gelu_tanh=gelu_tanh)
    H, W = 48, 64
    sd = vit_random_state_dict(cfg, 7, H, W)
    x = np.random.default_rng(3).uniform(-1, 1, (2, H, W, 3)).astype(np.float32)
    ref = vr.forward(sd, cfg, x)
    l64, l32 = torch_forward(sd, cfg, x, __import__("torch").float64), torch_forward(sd, cfg, x, __import__("torch").float32)
    e_torch = np.abs(l32 - l64).max()
    e_ref = np.abs(ref["logits"].astype(np.float64) - l64).max()
    print("tiny model (tanh=%d): torch fp32 vs fp64 %.3g, restatement vs fp64 %.3g, logits up to %.3g" % (gelu_tanh, e_torch, e_ref, np.abs(l64).max()))
    assert e_torch > 0 and e_ref <= 4 * e_torch
    assert ref["prob"].dtype == np.float32 and np.allclose(ref["prob"].sum(1), 1.0, atol=1e-6)
    assert np.array_equal(ref["topk_idx"], np.argsort(-ref["prob"], axis=1, kind="stable")[:, :cfg.topk])


def test_patch_weight_order_against_strided_conv():
    import torch
    from isegmi.vit import patch_weight_krsc
    rng = np.random.default_rng(0)
    for P, H, W in ((16, 32, 48), (32, 64, 32)):
        x = rng.standard_normal((2, H, W, 3)).astype(np.float32)
        w = rng.standard_normal((8, 3, P, P)).astype(np.float32)
        want = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(w.astype(np.float64)),
                                          stride=P).permute(0, 2, 3, 1).numpy()
        got = vr.patchify(x, P).astype(np.float64) @ patch_weight_krsc(w).reshape(8, -1).T.astype(np.float64)     # both sides in float64: only the order differs
        assert got.shape == want.shape == (2, H // P, W // P, 8) and np.allclose(got, want, rtol=0, atol=1e-11)
    with pytest.raises(ValueError, match="patch_embed.proj.weight"):
        patch_weight_krsc(np.zeros((8, 4, 16, 16), np.float32))


def test_config_validation_and_refusals_by_name():
    from isegmi.vit import VIT_VARIANTS, ViT, ViTConfig, vit_layers
    from isegmi.weights import vit_random_state_dict
    for name, (d, depth, heads, mlp, p) in VIT_VARIANTS.items():
        c = ViTConfig.named(name).validate()
        assert (c.dim, c.depth, c.heads, c.mlp_dim, c.patch, c.num_classes, c.ln_eps, c.gelu_tanh) == (d, depth, heads, mlp, p, 1000, 1e-6, False)
        assert c.tokens(224, 224) == (224 // p) ** 2 + 1
    assert ViTConfig.named("vit_b16").tokens(224, 224) == 197 and ViTConfig.named("vit_b16").validate(384, 384).tokens(384, 384) == 577
    for kw, H, W, key in ((dict(dim=256, heads=2), 224, 224, "heads"), (dict(patch=14), 224, 224, "patch"), (dict(), 230, 224, "height"), (dict(), 224, 100, "width"),
                          (dict(), 512, 528, "tokens"), (dict(num_classes=1), 224, 224, "num_classes"), (dict(num_classes=8193), 224, 224, "num_classes"),
                          (dict(topk=0), 224, 224, "topk"), (dict(topk=65), 224, 224, "topk"), (dict(ln_eps=-1.0), 224, 224, "ln_eps"),
                          (dict(mlp_dim=100), 224, 224, "mlp_dim"), (dict(depth=0), 224, 224, "depth")):
        with pytest.raises(ValueError, match=key):
            ViTConfig(**kw).validate(H, W)
    with pytest.raises(ValueError, match="vit_h14"):
        ViTConfig.named("vit_h14")
    cfg = tiny_cfg()
    sd = vit_random_state_dict(cfg, 1, 32, 32)
    with pytest.raises(ValueError, match="pos_embed.*not interpolated"):
        vit_layers(sd, cfg, 48, 48)
    with pytest.raises(ValueError, match="head.weight"):
        vit_layers(sd, tiny_cfg(num_classes=11), 32, 32)
    with pytest.raises(ValueError, match="cls_token: missing"):
        vit_layers({k: v for k, v in sd.items() if k != "cls_token"}, cfg, 32, 32)
    # refused before an engine (or a device) is touched
    with pytest.raises(ValueError, match="fp16"):
        ViT(sd, cfg, 32, 32, fp16=True)
    with pytest.raises(ValueError, match="graph"):
        ViT(sd, cfg, 32, 32, graph=True)
    with pytest.raises(ValueError, match="patch"):
        ViT(sd, ViTConfig(patch=14), 224, 224)
    convs, tensors = vit_layers(sd, cfg, 32, 32)
    assert convs["blocks.1.attn.qkv"][0].shape == (384, 1, 1, 128) and convs["patch_embed.proj"][0].shape == (128, 1, 1, 768)
    assert tensors["vit.pos_rows"].shape == (4, 128) and np.array_equal(tensors["vit.cls_row"], sd["cls_token"][0, 0] + sd["pos_embed"][0, 0])


def test_cli_arguments(monkeypatch):
    from isegmi.cli import build_parser, cmd_vit_classify, vit_config
    a = build_parser().parse_args(["vit_classify", "--images", "dir"])
    assert (a.model, a.weights, a.topk, a.output, a.num_classes, a.img_size, a.gelu_tanh, a.ln_eps) == ("vit_b16", "random", 5, "preds.json", 1000, 224, 0, 1e-6)
    c = vit_config(a)
    assert (c.dim, c.patch, c.topk, c.gelu_tanh) == (768, 16, 5, False)
    a = build_parser().parse_args(["vit_classify", "--model", "vit_b32", "--images", "d", "--topk", "3", "--gelu-tanh", "1", "--img-size", "384", "--num-classes", "21"])
    c = vit_config(a)
    assert (c.patch, c.topk, c.gelu_tanh, c.num_classes, c.tokens(384, 384)) == (32, 3, True, 21, 145)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["vit_classify", "--model", "vit_h14", "--images", "d"])
    with pytest.raises(ValueError, match="height"):
        vit_config(build_parser().parse_args(["vit_classify", "--images", "d", "--img-size", "230"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        cmd_vit_classify(build_parser().parse_args(["vit_classify", "--images", "d"]))
