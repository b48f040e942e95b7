"""The ViT engine (model kind 7) end to end against the composed reference of tests/vit_ref.py, bit for bit: a tiny model on three canvases (T = 5, 13 and
21 tokens: the last crosses a 16-row tile), both GELU forms, live parameters, vit_b16 at 224 once, and the command line."""
import json

import numpy as np
import pytest

import vit_ref as vr

pytestmark = pytest.mark.gpu
CANVASES = [(32, 32), (48, 64), (64, 80)]


def tiny_cfg(**kw):
    from isegmi.vit import ViTConfig
    return ViTConfig(**dict(dict(dim=128, depth=2, heads=2, mlp_dim=256, patch=16, num_classes=10, topk=3), **kw))


def images(n, H, W, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, H, W, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def tiny(ffi):
    """{canvas: (state dict, engine of max_batch 4, reference of a batch of 3)}, built on first use and shared: the reference is computed once"""
    from isegmi.vit import ViT
    from isegmi.weights import vit_random_state_dict
    made = {}

    def get(H, W):
        if (H, W) not in made:
            cfg = tiny_cfg()
            sd = vit_random_state_dict(cfg, 11, H, W)
            made[(H, W)] = (sd, ViT(sd, cfg, H, W, max_batch=4), vr.forward(sd, cfg, images(3, H, W)))
        return made[(H, W)]
    yield get
    for _, net, _ in made.values():
        net.close()


def check(out, ref, n):
    logits, prob, tv, ti = out
    for name, a, b in (("logits", logits, ref["logits"]), ("prob", prob, ref["prob"]), ("topk_val", tv, ref["topk_val"])):
        assert a.shape == b[:n].shape and np.array_equal(a.view(np.uint32), b[:n].view(np.uint32)), name
    assert np.array_equal(ti, ref["topk_idx"][:n])


@pytest.mark.parametrize("canvas", CANVASES)
def test_tiny_model_bit_exact(tiny, canvas):
    H, W = canvas
    sd, net, ref = tiny(H, W)
    x = images(3, H, W)
    out3 = net(x)
    check(out3, ref, 3)
    T = net.cfg.tokens(H, W)
    for name, want in (("vit.tokens", ref["tokens"]), ("vit.qkv", ref["blocks"][-1]["qkv"]), ("vit.attn", ref["blocks"][-1]["attn"]),
                       ("vit.mlp", ref["blocks"][-1]["mlp"])):
        got = net.fetch(name, 3).reshape(3, T, -1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    check(net(x[:1]), ref, 1)                       # batch 1 in the same engine: the same rows
    again = net(x)                                  # a second forward: identical bits
    assert all(np.array_equal(a, b) for a, b in zip(out3, again))


def test_gelu_forms_and_live_parameters(tiny):
    import dataclasses
    H, W = CANVASES[1]
    sd, net, ref = tiny(H, W)
    x = images(3, H, W)
    cfg = net.cfg
    try:
        net.configure(dataclasses.replace(cfg, gelu_tanh=True))
        t = net(x)
        check(t, vr.forward(sd, dataclasses.replace(cfg, gelu_tanh=True), x), 3)
        assert not np.array_equal(t[0], ref["logits"])
        net.configure(dataclasses.replace(cfg, topk=7))
        out = net(x)
        assert out[2].shape == (3, 7) and np.array_equal(out[3][:, :3], ref["topk_idx"]) and np.array_equal(out[0], ref["logits"])
        assert np.array_equal(out[3], np.argsort(-out[1], axis=1, kind="stable")[:, :7])
        with pytest.raises(ValueError, match="only topk"):
            net.configure(dataclasses.replace(cfg, depth=1))
    finally:
        net.configure(cfg)
    check(net(x), ref, 3)


def test_refusals_and_stage_marks(ffi, tiny):
    H, W = CANVASES[0]
    sd, net, ref = tiny(H, W)
    n = net.upload(images(1, H, W))
    for name, value, back in (("fp16", 1.0, 0.0), ("graph", 1.0, 0.0), ("vit_topk", 65.0, 3.0), ("vit_patch", 14.0, 16.0), ("vit_heads", 3.0, 2.0),
                              ("vit_num_classes", 1.0, 10.0), ("vit_gelu_tanh", 2.0, 0.0)):
        net.set_param(name, value)
        with pytest.raises(ffi.IsegmiError, match=name):
            net.forward_device(n)
        net.set_param(name, back)
    with pytest.raises(ffi.IsegmiError, match="not a yolact engine"):
        ffi.check(ffi.lib().isegmi_yolact_forward(net._h, net.input_buffer().ptr, 1))
    import ctypes as C
    h = C.c_void_p()
    for kind in (6, 8):            # ViT is kind 7; 6 stays refused, as tests/test_yolov3_gpu.py pins it
        with pytest.raises(ffi.IsegmiError, match="7 vit"):
            ffi.check(ffi.lib().isegmi_engine_create(kind, 1, 32, 32, C.byref(h)))
    net.set_param("timing", 1.0); net.set_param("conv_timing", 1.0)
    try:
        net.forward_device(n)
        net.sync()
        assert [s for s, _ in net.timings()] == ["embed", "blocks", "head"]
        flops, ms, launches = net.conv_stats()
        T, D, M, K = 5, 128, 256, 768
        assert launches == 1 + 4 * 2 + 1 and flops == 2.0 * ((T - 1) * K * D + 2 * T * (3 * D * D + D * D + 2 * D * M) + D * 10)
    finally:
        net.set_param("timing", 0.0); net.set_param("conv_timing", 0.0)
    check(net(images(3, H, W)), ref, 3)


def test_vit_b16_at_224(ffi):
    """vit_b16, one image: the embedding, block 0 (vit.attn and the block's output, from a forward cut at depth 1) and -- the reference forward of twelve
    blocks being too slow on the host -- the head applied to the device's final tokens."""
    from isegmi.vit import ViT, ViTConfig, vit_layers
    from isegmi.weights import vit_random_state_dict
    cfg = ViTConfig.named("vit_b16")
    sd = vit_random_state_dict(cfg, 5)
    x = images(1, 224, 224, 2)
    convs, tensors = vit_layers(sd, cfg, 224, 224)
    tokens = vr.embed(convs, tensors, cfg, x)
    b0 = vr.block(tokens, convs, tensors, 0, cfg)
    net = ViT(sd, cfg, 224, 224, max_batch=1)
    try:
        net.set_param("vit_depth", 1.0)             # the engine reads the depth at every forward: block 0 alone leaves its tensors in the named buffers
        net(x)
        net.set_param("vit_depth", float(cfg.depth))
        assert np.array_equal(net.fetch("vit.tokens", 1).view(np.uint32), tokens.view(np.uint32))
        assert np.array_equal(net.fetch("vit.attn", 1).reshape(1, 197, 768).view(np.uint32), b0["attn"].view(np.uint32))
        assert np.array_equal(net.fetch("vit.x2", 1).reshape(1, 197, 768).view(np.uint32), b0["x"].view(np.uint32))
        logits, prob, tv, ti = net(x)
        final = net.fetch("vit.x2", 1).reshape(1, 197, 768)
        want = vr.head(final, convs, tensors, cfg)
        assert np.isfinite(final).all()
        for a, b in zip((logits, prob, tv), want[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(ti, want[3])
    finally:
        net.close()


def test_vit_classify_end_to_end(ffi, tmp_path):
    from PIL import Image
    from isegmi.cli import main
    rng = np.random.default_rng(1)
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate(((40, 56), (64, 64), (90, 33))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(d / ("im%d.png" % i)))
    out = tmp_path / "preds.json"
    res = main(["vit_classify", "--model", "vit_ti16", "--weights", "random", "--images", str(d), "--img-size", "64", "--topk", "4", "--num-classes", "12",
                "--output", str(out), "--batch-size", "2"])
    disk = json.load(open(str(out)))
    assert disk == res and [r["file"] for r in disk] == ["im0.png", "im1.png", "im2.png"]
    for r in disk:
        assert len(r["labels"]) == len(r["probabilities"]) == 4 and len(set(r["labels"])) == 4 and all(0 <= v < 12 for v in r["labels"])
        assert r["probabilities"] == sorted(r["probabilities"], reverse=True) and 0 < sum(r["probabilities"]) <= 1 + 1e-6
    # the 64 x 64 image needs no resize: the front end is (x - 127.5) / 127.5 in RGB order, and the engine's bits are the reference's
    from isegmi.vit import ViTConfig
    from isegmi.weights import vit_random_state_dict
    cfg = ViTConfig.named("vit_ti16", num_classes=12, topk=4)
    im = np.asarray(Image.open(str(d / "im1.png")).convert("RGB"), np.float32)
    ref = vr.forward(vit_random_state_dict(cfg, 1234, 64, 64), cfg, ((im - np.float32(127.5)) / np.float32(127.5))[None])
    assert disk[1]["labels"] == ref["topk_idx"][0].tolist() and disk[1]["probabilities"] == [float(v) for v in ref["topk_val"][0]]
