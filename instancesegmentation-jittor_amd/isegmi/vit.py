"""ViT inference, host side ([UPSTREAM-RECALL] the ViT of Dosovitskiy et al. in the PyTorch / timm layout, unverified: the reference's
ViT.jittor directory is empty).  `net = ViT(sd, cfg, H, W)`; `net(batch)` -> (logits [n, classes], prob [n, classes], top-k values [n, k], top-k
indices [n, k]).  `ViTClassifier(...).classify(images)` adds the device front end (resize, normalisation).  All numerics run in libisegmi.so (engine
kind 7); this module moves config, weights and results across the C ABI."""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .engine import Engine

VIT_HEAD_DIM = 64       # csrc/vit_ops.hip AT_HD
VIT_MAX_TOKENS = 1024
VIT_MAX_CLASSES = 8192
VIT_MAX_TOPK = 64
# name: (dim, depth, heads, mlp_dim, patch)
VIT_VARIANTS = {"vit_ti16": (192, 12, 3, 768, 16), "vit_s16": (384, 12, 6, 1536, 16), "vit_b16": (768, 12, 12, 3072, 16),
                "vit_b32": (768, 12, 12, 3072, 32), "vit_l16": (1024, 24, 16, 4096, 16)}


@dataclass(frozen=True)
class ViTConfig:
    """dim = 64 * heads.  gelu_tanh False: the exact erf GELU (PyTorch, timm); True: the tanh form of the original JAX release.  ln_eps: 1e-6 (timm);
    torch.nn.LayerNorm's own default is 1e-5."""
    dim: int = 768
    depth: int = 12
    heads: int = 12
    mlp_dim: int = 3072
    patch: int = 16
    num_classes: int = 1000
    ln_eps: float = 1e-6
    gelu_tanh: bool = False
    topk: int = 5

    @classmethod
    def named(cls, name, **kw):
        if name not in VIT_VARIANTS:
            raise ValueError("model=%r: one of %s" % (name, ", ".join(sorted(VIT_VARIANTS))))
        d, depth, heads, mlp, p = VIT_VARIANTS[name]
        return cls(dim=d, depth=depth, heads=heads, mlp_dim=mlp, patch=p, **kw)

    def tokens(self, H, W):
        return (H // self.patch) * (W // self.patch) + 1

    def validate(self, H=224, W=224):
        """Raises ValueError naming the key that is refused."""
        if self.heads < 1 or self.dim != VIT_HEAD_DIM * self.heads:
            raise ValueError("dim=%d, heads=%d: the head dimension dim / heads must be exactly %d" % (self.dim, self.heads, VIT_HEAD_DIM))
        if self.depth < 1:
            raise ValueError("depth=%d: at least one block" % self.depth)
        if self.mlp_dim < 32 or self.mlp_dim % 32:
            raise ValueError("mlp_dim=%d: a positive multiple of 32" % self.mlp_dim)
        if self.patch not in (16, 32):
            raise ValueError("patch=%d: 16 or 32 (3 * patch^2 must be a multiple of 32; patch 14 is not built)" % self.patch)
        for key, v in (("height", H), ("width", W)):
            if v <= 0 or v % self.patch:
                raise ValueError("%s=%d: canvas sides are positive multiples of patch=%d" % (key, v, self.patch))
        if self.tokens(H, W) > VIT_MAX_TOKENS:
            raise ValueError("height=%d, width=%d: %d tokens, the attention kernel holds %d" % (H, W, self.tokens(H, W), VIT_MAX_TOKENS))
        if not 2 <= self.num_classes <= VIT_MAX_CLASSES:
            raise ValueError("num_classes=%d: 2..%d" % (self.num_classes, VIT_MAX_CLASSES))
        if not self.ln_eps >= 0:
            raise ValueError("ln_eps=%r: a non-negative number" % (self.ln_eps,))
        if not 1 <= self.topk <= min(VIT_MAX_TOPK, self.num_classes):
            raise ValueError("topk=%d: 1..min(%d, num_classes)" % (self.topk, VIT_MAX_TOPK))
        return self


def patch_weight_krsc(w_oihw):
    """patch_embed.proj.weight [D][3][P][P] -> [D][1][1][P * P * 3] in (py, px, c) order: the K order of isegmi_op_patchify."""
    w = np.asarray(w_oihw, np.float32)
    d, c, p, p2 = w.shape
    if c != 3 or p != p2:
        raise ValueError("patch_embed.proj.weight: expected [D][3][P][P], got %s" % (w.shape,))
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(d, 1, 1, p * p * 3)


def vit_layers(sd, cfg, H, W):
    """-> (convs {name: (w [Cout][1][1][Cin], bias)}, tensors {name: array}) of a timm-layout state dict; every shape is checked by name."""
    D, T = cfg.dim, cfg.tokens(H, W)

    def get(name, shape):
        if name not in sd:
            raise ValueError("%s: missing from the state dict" % name)
        a = np.asarray(sd[name], np.float32)
        if a.shape != tuple(shape):
            hint = " (the position embedding is not interpolated: H / patch * W / patch + 1 = %d tokens)" % T if name == "pos_embed" else ""
            raise ValueError("%s: expected %s, got %s%s" % (name, tuple(shape), a.shape, hint))
        return a

    def linear(name, cout, cin):
        return get(name + ".weight", (cout, cin)).reshape(cout, 1, 1, cin), get(name + ".bias", (cout,))

    convs = {"patch_embed.proj": (patch_weight_krsc(get("patch_embed.proj.weight", (D, 3, cfg.patch, cfg.patch))), get("patch_embed.proj.bias", (D,)))}
    tensors = {}
    for i in range(cfg.depth):
        b = "blocks.%d." % i
        convs[b + "attn.qkv"] = linear(b + "attn.qkv", 3 * D, D)
        convs[b + "attn.proj"] = linear(b + "attn.proj", D, D)
        convs[b + "mlp.fc1"] = linear(b + "mlp.fc1", cfg.mlp_dim, D)
        convs[b + "mlp.fc2"] = linear(b + "mlp.fc2", D, cfg.mlp_dim)
        for nm in ("norm1", "norm2"):
            tensors[b + nm + ".weight"], tensors[b + nm + ".bias"] = get(b + nm + ".weight", (D,)), get(b + nm + ".bias", (D,))
    tensors["norm.weight"], tensors["norm.bias"] = get("norm.weight", (D,)), get("norm.bias", (D,))
    convs["head"] = linear("head", cfg.num_classes, D)
    pos = get("pos_embed", (1, T, D))[0]
    tensors["vit.cls_row"] = get("cls_token", (1, 1, D))[0, 0] + pos[0]      # one fp32 addition per channel
    tensors["vit.pos_rows"] = pos[1:]
    return convs, tensors


class ViT(Engine):
    KIND = 7

    def __init__(self, state_dict, cfg=ViTConfig(), H=224, W=224, max_batch=8, device=0, fp16=False, graph=False):
        if fp16:
            raise ValueError("ViT: fp16=True is not built (fp32 only)")
        if graph:
            raise ValueError("ViT: graph=True (hipGraph capture) is not built")
        H, W = int(H), int(W)
        cfg.validate(H, W)
        convs, tensors = vit_layers(state_dict, cfg, H, W)
        self.cfg, self.H, self.W, self.max_batch = cfg, H, W, max_batch
        self.fp16 = False
        self._create(device, max_batch, H, W)
        for name, (w, b) in convs.items():
            self._set_conv_krsc(name, w, None, b)
        tensors["vit.pos_rows"] = np.tile(tensors["vit.pos_rows"][None], (max_batch, 1, 1))
        for name, a in tensors.items():
            self._set_tensor(name, np.ascontiguousarray(a, np.float32))
        self.configure(cfg)
        self._d_in = _ffi.DeviceBuffer((max_batch, H, W, 3))

    def configure(self, cfg):
        """The parameters from a config.  topk, gelu_tanh and ln_eps are live (the next forward uses them); the shape must stay the weights'."""
        cfg.validate(self.H, self.W)
        if dataclasses.replace(cfg, topk=self.cfg.topk, gelu_tanh=self.cfg.gelu_tanh, ln_eps=self.cfg.ln_eps) != self.cfg:
            raise ValueError("configure: only topk, gelu_tanh and ln_eps change on a live engine")
        for k, v in (("vit_dim", cfg.dim), ("vit_depth", cfg.depth), ("vit_heads", cfg.heads), ("vit_mlp_dim", cfg.mlp_dim), ("vit_patch", cfg.patch),
                     ("vit_num_classes", cfg.num_classes), ("vit_ln_eps", cfg.ln_eps), ("vit_gelu_tanh", float(bool(cfg.gelu_tanh))), ("vit_topk", cfg.topk)):
            self.set_param(k, float(v))
        self.cfg = cfg

    def upload(self, batch_nhwc3, slot=0):
        """A normalised fp32 batch [n, H, W, 3]."""
        x = np.ascontiguousarray(batch_nhwc3, np.float32)
        assert x.ndim == 4 and x.shape[1:] == (self.H, self.W, 3) and x.shape[0] <= self.max_batch, x.shape
        _ffi.check(_ffi.lib().isegmi_h2d(self.input_buffer(slot).ptr, x.ctypes.data_as(C.c_void_p), x.nbytes))
        return x.shape[0]

    def forward_device(self, n, slot=0):
        _ffi.check(_ffi.lib().isegmi_vit_forward(self._h, self.input_buffer(slot).ptr, n))

    def results(self, n):
        """(logits [n, classes], prob [n, classes], top-k probabilities [n, k], top-k class indices [n, k]) of the last forward."""
        return tuple(self.fetch(k, n) for k in ("cls.logits", "cls.prob", "cls.topk_val", "cls.topk_idx"))

    def __call__(self, batch_nhwc3):
        n = self.upload(batch_nhwc3)
        self.forward_device(n)
        self.sync()
        return self.results(n)


VIT_MEAN = VIT_STD = (127.5, 127.5, 127.5)   # the "inception" normalisation of the published checkpoints: x / 127.5 - 1


class ViTClassifier:
    """Images in, (labels [k], probabilities [k]) per image out: bilinear resize to the canvas and normalisation on the device (isegmi_op_preprocess_u8;
    RGB order, (x - 127.5) / 127.5), ViT on the device.  `logits` holds the raw logits of the last classify call, one row per image."""

    def __init__(self, state_dict, cfg=ViTConfig(), H=224, W=224, max_batch=8, device=0):
        self.cfg = cfg
        self.net = ViT(state_dict, cfg, H, W, max_batch=max_batch, device=device)
        self.logits = None

    def classify(self, images_bgr_u8):
        """list of HxWx3 uint8 BGR images -> list of (labels [k] int32, probabilities [k] float32), best first."""
        net, out, logits = self.net, [], []
        for i0 in range(0, len(images_bgr_u8), net.max_batch):
            ims = images_bgr_u8[i0:i0 + net.max_batch]
            for j, im in enumerate(ims):     # one front-end launch per image: the sources differ in size
                im = np.ascontiguousarray(im, np.uint8)
                assert im.ndim == 3 and im.shape[2] == 3, im.shape
                st = net._u8_staging(0, im.nbytes)
                net.sync()                   # the staging buffer is reused image by image
                _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, im.ctypes.data_as(C.c_void_p), im.nbytes))
                dst = net.input_buffer(0).ptr.value + j * net.H * net.W * 3 * 4
                net._preprocess_u8(st.ptr.value, 1, im.shape[0], im.shape[1], dst, net.H, net.W, net.H, net.W, VIT_MEAN, VIT_STD, True)
            net.forward_device(len(ims))
            net.sync()
            lg, _, tv, ti = net.results(len(ims))
            logits.append(lg)
            out += [(ti[j].copy(), tv[j].copy()) for j in range(len(ims))]
        self.logits = np.concatenate(logits) if logits else np.zeros((0, self.cfg.num_classes), np.float32)
        return out

    def close(self):
        self.net.close()
