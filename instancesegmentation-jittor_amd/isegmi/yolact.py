"""Yolact R50-FPN inference, host side (mirrors Yolact.jittor's eval surface).

Reference surface (README.md:243-249): `python eval.py --trained_model=... --score_threshold=0.15
--top_k=15 --image=...` -> [UPSTREAM-RECALL, SURVEY 8b] `net(batch) -> [{'detection': {'box','mask',
'class','score','proto'}, 'net'}]` and `postprocess(dets, w, h, score_threshold) -> (classes, scores,
boxes, masks)`.  Everything numeric runs in libisegmi.so (HIP); this file only moves config,
weights and results across the C ABI.
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .engine import Engine
from .weights import dcn_blocks, fold_batchnorm, to_krsc

MEANS = (103.94, 116.78, 123.68)  # BGR
STD = (57.38, 57.12, 58.40)


@dataclass(frozen=True)
class YolactConfig:
    """yolact_resnet50_config constants."""
    max_size: int = 550
    num_classes: int = 81
    mask_dim: int = 32
    pred_scales: tuple = (24, 48, 96, 192, 384)
    pred_aspect_ratios: tuple = (1.0, 0.5, 2.0)
    nms_conf_thresh: float = 0.05
    nms_thresh: float = 0.5
    nms_top_k: int = 200
    max_num_detections: int = 100
    nms_second_threshold: int = 0  # SURVEY App. A.6 fork: Detect.fast_nms(second_threshold=True) -- a box must also have its own class score > nms_conf_thresh
    # the suppression rule, upstream's names (Detect: cfg.use_fast_nms / cfg.use_cross_class_nms; eval.py --fast_nms / --cross_class_nms)
    use_fast_nms: bool = True          # False: traditional per-class NMS (cython_nms), "--fast_nms=False"
    use_cross_class_nms: bool = False  # True (with use_fast_nms): one fast-NMS pass over all classes together
    nms_trad_cap: int = 1024           # traditional NMS visits at most this many candidates per (image, class); a multiple of 64 in [64, 2048]
    conv_split_k: int = 0          # opt-in latency numerics mode (see MaskRCNNConfig.CONV_SPLIT_K): fixed-tree split-K for the backbone's small-M / large-K convolutions
    depth: int = 50  # 50 = yolact_resnet50_config, 101 = yolact_base_config / yolact_im700_config
    # YOLACT++ (yolact_plus_*_config, the YOLACT++ rows of README.md:216-221): three scales per level x three aspect ratios,
    # rectangular anchors, DCNv2 3x3s in the backbone, fast mask re-scoring
    scales_per_level: int = 1          # 3: scale * 2**(j/3), j = 0..2
    use_square_anchors: bool = True
    dcn_layers: tuple = (0, 0, 0, 0)
    dcn_interval: int = 1
    use_maskiou: bool = False
    backbone: str = "resnet"           # "darknet53": yolact_darknet53_config (DarkNetBackbone([1, 2, 8, 8, 4]), LeakyReLU(0.1))

    def __post_init__(self):
        for k in ("use_fast_nms", "use_cross_class_nms"):
            if not isinstance(getattr(self, k), (bool, np.bool_)):
                raise TypeError("YolactConfig.%s must be a bool, got %r" % (k, getattr(self, k)))
        cap = self.nms_trad_cap
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 64 or cap > 2048 or cap % 64:
            raise ValueError("YolactConfig.nms_trad_cap must be a multiple of 64 in [64, 2048], got %r" % (cap,))
        if self.nms_second_threshold and self.nms_mode != 0:
            raise ValueError("YolactConfig.nms_second_threshold is an argument of fast_nms only: it cannot be combined with "
                             "use_cross_class_nms=True or use_fast_nms=False")

    @property
    def nms_mode(self):
        """The engine's `nms_mode`, chosen as upstream Detect.detect() chooses: 0 fast_nms, 1 cc_fast_nms, 2 traditional_nms."""
        return nms_mode_of(self.use_fast_nms, self.use_cross_class_nms, warn=False)

    @property
    def num_priors(self):
        return self.scales_per_level * len(self.pred_aspect_ratios)

    def level_scales(self, level):
        s = self.pred_scales[level]
        return tuple(s * 2 ** (j / 3.0) for j in range(self.scales_per_level))

    @staticmethod
    def darknet53():
        """yolact_darknet53_config: Darknet53-FPN at 550 (same heads / anchors as the ResNet configs; upstream preprocesses with
        darknet_transform: RGB, x / 255, no mean / std)."""
        return YolactConfig(backbone="darknet53")

    @staticmethod
    def plus_base():
        """yolact_plus_base_config: ResNet101-FPN with a DCNv2 every third block of layers 2-4 (resnet101_dcn_inter3_backbone)."""
        return YolactConfig(depth=101, scales_per_level=3, use_square_anchors=False, dcn_layers=(0, 4, 23, 3), dcn_interval=3,
                            use_maskiou=True)

    @staticmethod
    def plus_resnet50():
        """yolact_plus_resnet50_config: ResNet50-FPN with DCNv2 in every block of layers 2-4 (resnet50_dcnv2_backbone)."""
        return YolactConfig(depth=50, scales_per_level=3, use_square_anchors=False, dcn_layers=(0, 4, 6, 3), dcn_interval=1,
                            use_maskiou=True)

    @staticmethod
    def base():
        """yolact_base_config: ResNet101-FPN at 550."""
        return YolactConfig(depth=101)

    @staticmethod
    def im700():
        """yolact_im700_config: ResNet101-FPN at 700, pred_scales = int(s / 550 * 700)."""
        return YolactConfig(max_size=700, pred_scales=tuple(int(s / 550 * 700) for s in (24, 48, 96, 192, 384)), depth=101)


def nms_mode_of(use_fast_nms, use_cross_class_nms, warn=True):
    """Upstream Detect.detect(): `if cfg.use_cross_class_nms: cc_fast_nms` / `elif cfg.use_fast_nms: fast_nms` / `else: traditional_nms`, where
    traditional_nms asserts (here: warns, as eval.py's users see it) that a cross-class traditional NMS does not exist and runs per class."""
    if use_fast_nms:
        return 1 if use_cross_class_nms else 0
    if use_cross_class_nms and warn:
        import warnings
        warnings.warn("cross-class traditional NMS is not implemented (upstream has none either): running traditional per-class NMS")
    return 2


class NmsCapOverflow(RuntimeError):
    """Traditional NMS met a class with more candidates than nms_trad_cap in a way that can change the result: raise nms_trad_cap."""


def make_priors(conv_h, conv_w, scales, max_size, ars, square=True):
    """PredictionModule.make_priors with use_pixel_scales, preapply_sqrt=False: per cell, scale-major / ratio-minor."""
    scales = tuple(scales) if isinstance(scales, (tuple, list)) else (scales,)
    out = np.empty((conv_h, conv_w, len(scales) * len(ars), 4), np.float64)
    xs = (np.arange(conv_w) + 0.5) / conv_w
    ys = (np.arange(conv_h) + 0.5) / conv_h
    out[..., 0] = xs[None, :, None]
    out[..., 1] = ys[:, None, None]
    a = 0
    for scale in scales:
        for ar in ars:
            r = math.sqrt(ar)
            w = scale * r / max_size
            out[..., a, 2] = w
            out[..., a, 3] = w if square else scale / r / max_size
            a += 1
    return out.reshape(-1, 4).astype(np.float32)


def darknet_base_transform(images_bgr_u8):
    """FastBaseTransform under darknet_transform (yolact_darknet53_config): x / 255, then BGR -> RGB; no mean / std.  NHWC3 fp32."""
    x = np.asarray(images_bgr_u8, np.float32) / np.float32(255.0)
    return np.ascontiguousarray(x[..., ::-1])


def fast_base_transform(images_bgr_u8):
    """FastBaseTransform for already-550x550 BGR uint8 images (Y1): (x-mean)/std then BGR->RGB. NHWC3 fp32."""
    x = np.asarray(images_bgr_u8, np.float32)
    x = (x - np.asarray(MEANS, np.float32)) / np.asarray(STD, np.float32)
    return np.ascontiguousarray(x[..., ::-1])


def _level_sizes(size):
    s = (size + 6 - 7) // 2 + 1      # conv1 7x7/2 p3
    s = (s + 2 - 3) // 2 + 1         # maxpool 3/2/1
    c3 = (s + 2 - 3) // 2 + 1        # layer2 stride 2 (3x3 p1)
    c4 = (c3 + 2 - 3) // 2 + 1
    c5 = (c4 + 2 - 3) // 2 + 1
    p6 = (c5 + 2 - 3) // 2 + 1
    p7 = (p6 + 2 - 3) // 2 + 1
    return [c3, c4, c5, p6, p7]


class Yolact(Engine):
    """`net = Yolact(state_dict); preds = net(batch)`; `postprocess(preds, w, h, score_threshold)`."""

    KIND = 1

    def __init__(self, state_dict, cfg=YolactConfig(), max_batch=8, device=0, input_size=None, fuse_heads=True, fp16=False):
        """fp16=True: optional fp16-storage / f16-MFMA mode (backbone, FPN, protonet and head convolutions; the fused head
        outputs, the prototypes and Detect / mask assembly stay fp32).  Not bit-exact: tolerance parity vs YolactRef(fp16=True)."""
        assert not fp16 or fuse_heads, "fp16 Yolact uses the fused prediction head"
        self.fp16 = bool(fp16)
        self.cfg = cfg
        self.size = int(input_size or cfg.max_size)
        self.max_batch = max_batch
        self.fuse_heads = bool(fuse_heads)
        self._create(device, max_batch, self.size, self.size)
        self.set_param("resnet_depth", float(cfg.depth))
        self.set_param("num_priors", float(cfg.num_priors))
        self.set_param("darknet", 1.0 if cfg.backbone == "darknet53" else 0.0)
        assert not (fp16 and cfg.backbone == "darknet53"), "the Darknet53 backbone runs in fp32 only"
        assert not (fp16 and any(cfg.dcn_layers)), "the DCNv2 backbones run in fp32 only"
        if self.fp16:  # must precede weight loading (weights are packed as fp16)
            self.set_param("fp16", 1.0)
        self._load(state_dict)
        for k in ("nms_conf_thresh", "nms_thresh", "nms_top_k", "max_num_detections", "nms_second_threshold", "conv_split_k"):
            self.set_param(k, float(getattr(cfg, k)))
        mode = nms_mode_of(cfg.use_fast_nms, cfg.use_cross_class_nms)
        if mode:  # the default mode sets nothing: its parameter table is what it was
            self.set_param("nms_mode", float(mode))
            self.set_param("nms_trad_cap", float(cfg.nms_trad_cap))
            self.set_param("max_size", float(cfg.max_size))   # traditional NMS runs on boxes * cfg.max_size, as upstream scales them
        self._d_in = _ffi.DeviceBuffer((max_batch, self.size, self.size, 3))
        self._forward_id = 0
        self._pp_key = None

    @property
    def nms_mode(self):
        """the engine's current `nms_mode` parameter (0 fast, 1 cross-class fast, 2 traditional): read back from the engine, so a caller
        who switches the mode with set_param is checked by check_nms_overflow as one who chose it in the config"""
        return int(self.param("nms_mode", 0))

    @property
    def nms_trad_cap(self):
        """the engine's current `nms_trad_cap` parameter (1024, the engine's default, while nothing has set it)"""
        return int(self.param("nms_trad_cap", 1024))

    # -- weights -------------------------------------------------------------------------------
    def _set_conv(self, name, w_oihw, scale=None, shift=None, pad_cin_to=None):
        w = to_krsc(w_oihw)
        if pad_cin_to and w.shape[3] < pad_cin_to:
            w = np.concatenate([w, np.zeros(w.shape[:3] + (pad_cin_to - w.shape[3],), np.float32)], -1)
        self._set_conv_krsc(name, w, scale, shift)

    def _load(self, sd):
        dcn = dcn_blocks(self.cfg.depth, self.cfg.dcn_layers, self.cfg.dcn_interval)
        if self.cfg.backbone == "darknet53":
            sc, sh = fold_batchnorm(sd, "backbone._preconv.1")
            self._set_conv("backbone._preconv.0", sd["backbone._preconv.0.weight"], sc, sh, pad_cin_to=32)
            for li, nb in enumerate((1, 2, 8, 8, 4)):
                nm = "backbone.layers.%d" % li
                sc, sh = fold_batchnorm(sd, nm + ".0.1")
                self._set_conv(nm + ".0.0", sd[nm + ".0.0.weight"], sc, sh)
                for b in range(1, nb + 1):
                    for i in (1, 2):
                        sc, sh = fold_batchnorm(sd, "%s.%d.bn%d" % (nm, b, i))
                        self._set_conv("%s.%d.conv%d" % (nm, b, i), sd["%s.%d.conv%d.weight" % (nm, b, i)], sc, sh)
        else:
            self._load_resnet(sd, dcn)
        self._load_heads(sd)

    def _load_resnet(self, sd, dcn):
        sc, sh = fold_batchnorm(sd, "backbone.bn1")
        self._set_conv("backbone.conv1", sd["backbone.conv1.weight"], sc, sh, pad_cin_to=4)
        for li, nb in enumerate((3, 4, 23 if self.cfg.depth == 101 else 6, 3)):
            for b in range(nb):
                nm = "backbone.layers.%d.%d" % (li, b)
                for i in (1, 2, 3):
                    sc, sh = fold_batchnorm(sd, "%s.bn%d" % (nm, i))
                    w = sd["%s.conv%d.weight" % (nm, i)]
                    if i == 2 and (li, b) in dcn:
                        # DCNv2: the engine samples the 9 taps into columns (isegmi_op_deform_im2col) and runs the 3x3 as a 1x1 over
                        # 9*Cin channels in KRSC order -- the same k-ordered chain; the DCN bias folds into the BN shift
                        k = to_krsc(w)
                        w = k.reshape(k.shape[0], 1, 1, -1).transpose(0, 3, 1, 2)
                        sh = (sh + sd[nm + ".conv2.bias"].astype(np.float32) * sc).astype(np.float32)
                        self._set_conv(nm + ".conv2.conv_offset_mask", sd[nm + ".conv2.conv_offset_mask.weight"], None,
                                       sd[nm + ".conv2.conv_offset_mask.bias"])
                    self._set_conv("%s.conv%d" % (nm, i), w, sc, sh)
                if b == 0:
                    sc, sh = fold_batchnorm(sd, nm + ".downsample.1")
                    self._set_conv(nm + ".downsample.0", sd[nm + ".downsample.0.weight"], sc, sh)

    def _load_heads(self, sd):
        biased = ["fpn.lat_layers.%d" % i for i in range(3)] + ["fpn.pred_layers.%d" % i for i in range(3)] + \
                 ["fpn.downsample_layers.%d" % i for i in range(2)] + ["proto_net.%d" % i for i in (0, 2, 4, 8, 10)] + \
                 ["prediction_layers.0." + n for n in ("upfeature.0", "bbox_layer", "conf_layer", "mask_layer")]
        for nm in biased:
            self._set_conv(nm, sd[nm + ".weight"], None, sd[nm + ".bias"])
        # fused prediction head: [A*4 loc | A*81 conf | A*32 mask] as one 351-wide conv (tanh moves to the gather)
        if self.fuse_heads:
            names = ["prediction_layers.0." + n for n in ("bbox_layer", "conf_layer", "mask_layer")]
            self._set_conv("prediction_layers.0.head_cat", np.concatenate([sd[n + ".weight"] for n in names], 0), None,
                           np.concatenate([sd[n + ".bias"] for n in names]))
        self.has_maskiou = bool(self.cfg.use_maskiou and "maskiou_net.0.weight" in sd)  # a checkpoint without the net: box scores only
        if self.has_maskiou:
            # FastMaskIoUNet: layer 0 (one input channel) goes over as plain tensors for its dedicated kernel; layers 2..8 and the
            # 1x1 run on the MFMA conv kernels with channels padded to 32 by ZERO weights / biases (exact: the extra terms are +-0)
            w0 = to_krsc(sd["maskiou_net.0.weight"]).reshape(8, 9)
            for nm, arr in (("maskiou.w0", w0), ("maskiou.b0", sd["maskiou_net.0.bias"])):
                self._set_tensor(nm, np.ascontiguousarray(arr, np.float32))
            for i in (2, 4, 6, 8, 10):
                w = np.asarray(sd["maskiou_net.%d.weight" % i], np.float32); bias = np.asarray(sd["maskiou_net.%d.bias" % i], np.float32)
                cout, cin = w.shape[:2]
                cin_p = max(32, cin); cout_p = max(32, cout) if i != 10 else cout
                wp = np.zeros((cout_p, cin_p) + w.shape[2:], np.float32); wp[:cout, :cin] = w
                bp = np.zeros(cout_p, np.float32); bp[:cout] = bias
                self._set_conv("maskiou_net.%d" % i, wp, None, bp)
        pri = [make_priors(s, s, self.cfg.level_scales(l), self.cfg.max_size, self.cfg.pred_aspect_ratios, self.cfg.use_square_anchors)
               for l, s in enumerate(_level_sizes(self.size))]
        self.priors = np.concatenate(pri, 0)
        self._set_tensor("priors", self.priors)

    # -- execution -----------------------------------------------------------------------------
    def upload(self, batch_nhwc3):
        x = np.ascontiguousarray(batch_nhwc3, np.float32)
        assert x.ndim == 4 and x.shape[1:] == (self.size, self.size, 3) and x.shape[0] <= self.max_batch, x.shape
        _ffi.check(_ffi.lib().isegmi_h2d(self._d_in.ptr, x.ctypes.data_as(C.c_void_p), x.nbytes))
        return x.shape[0]

    def _u8_norm(self):
        darknet = self.cfg.backbone == "darknet53"
        return ((0.0, 0.0, 0.0), (255.0, 255.0, 255.0)) if darknet else (MEANS, STD)

    def upload_u8(self, images_bgr_u8, slot=0):
        """FastBaseTransform on the device (Y1): uint8 BGR images -- an [N, H, W, 3] array or a list of HxWx3 arrays of DIFFERENT sizes --
        -> bilinear resize to the network size, the backbone's normalisation, RGB: bit-identical to isegmi.transforms.yolact_transform
        on the host, a quarter of the PCIe bytes (and none of the host's resize arithmetic).  The previous forward on this input slot
        must have completed, as for upload()."""
        ims = self._as_u8_list(images_bgr_u8)
        flat = ims[0].reshape(-1) if len(ims) == 1 else np.concatenate([im.reshape(-1) for im in ims])
        st = self._u8_staging(slot, flat.nbytes)
        _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, flat.ctypes.data_as(C.c_void_p), flat.nbytes))
        self._front_end(st, [im.shape[:2] for im in ims], slot)
        return len(ims)

    def _as_u8_list(self, images):
        if isinstance(images, np.ndarray) and images.ndim == 4:
            images = [images[i] for i in range(images.shape[0])] if images.shape[0] != 1 else [images[0]]
        ims = [np.ascontiguousarray(im) for im in images]
        if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in ims):
            raise TypeError("upload_u8 takes HxWx3 uint8 images: a float batch is the already-transformed input of upload()")
        assert 0 < len(ims) <= self.max_batch, len(ims)
        return ims

    def _front_end(self, st, sizes_hw, slot):
        """image i of the staging buffer (back to back, each h x w x 3) -> plane i of the network input; equal sizes go as one launch"""
        mean, std = self._u8_norm()
        d_out = self.input_buffer(slot).ptr.value
        plane = self.size * self.size * 3 * 4
        sizes = [(int(h), int(w)) for h, w in sizes_hw]
        if len(set(sizes)) == 1:
            h, w = sizes[0]
            self._preprocess_u8(st.ptr.value, len(sizes), h, w, d_out, self.size, self.size, self.size, self.size, mean, std, True)
            return
        off = 0
        for i, (h, w) in enumerate(sizes):
            self._preprocess_u8(st.ptr.value + off, 1, h, w, d_out + i * plane, self.size, self.size, self.size, self.size, mean, std, True)
            off += h * w * 3

    def upload_u8_async(self, pinned_u8, n, h=None, w=None, slot=0, sizes_hw=None):
        """upload_u8 from a uint8 _ffi.PinnedBuffer holding the images back to back, on the engine's copy stream (see upload_async for
        the ordering): n images of one size (h, w), or sizes_hw = [(h, w), ...] per image."""
        sizes = [(int(h), int(w))] * n if sizes_hw is None else [(int(a), int(b)) for a, b in sizes_hw]
        nbytes = sum(a * b * 3 for a, b in sizes)
        assert pinned_u8.nbytes >= nbytes and len(sizes) <= self.max_batch
        st = self._u8_staging(slot, nbytes)
        _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, st.ptr, pinned_u8.ptr, nbytes))
        self._front_end(st, sizes, slot)

    def forward_device(self, n, slot=0):
        """Launch forward on the batch already resident in the engine's input buffer (asynchronous)."""
        self._pp_key = None  # masks / integer boxes cached by postprocess() belong to the previous forward
        self._forward_id += 1
        _ffi.check(_ffi.lib().isegmi_yolact_forward(self._h, self.input_buffer(slot).ptr, n))

    def postprocess_device(self, h, w):
        _ffi.check(_ffi.lib().isegmi_yolact_postprocess(self._h, h, w))

    def postprocess_device_sizes(self, image_hw):
        """postprocess with image n assembled at ITS (h, w) = image_hw[n] inside a common plane of the batch's maximum size."""
        hw = np.ascontiguousarray(image_hw, np.int32).reshape(-1, 2)
        _ffi.check(_ffi.lib().isegmi_yolact_postprocess_sizes(self._h, hw.ctypes.data_as(C.c_void_p), hw.shape[0]))

    def __call__(self, batch_nhwc3):
        """Upstream-shaped result: list (one per image) of {'detection': {...}|None, 'net': self}.  A uint8 [N, H, W, 3] batch is taken as
        raw BGR images of any one size and goes through the device front end (upload_u8: FastBaseTransform on the GPU); a float batch is
        the already-transformed network input."""
        raw = isinstance(batch_nhwc3, (list, tuple)) or np.asarray(batch_nhwc3).dtype == np.uint8
        n = self.upload_u8(batch_nhwc3) if raw else self.upload(batch_nhwc3)
        self.forward_device(n)
        self.sync()
        cnt = self.fetch("det.count", n)
        total = self.check_nms_overflow(n)
        box, score, cls, coeff, prior = (self.fetch(k, n) for k in ("det.box", "det.score", "det.class", "det.coeff", "det.prior"))
        proto = self.fetch("proto", n)
        out = []
        for i in range(n):
            c = int(cnt[i])
            det = None if c == 0 else dict(box=box[i, :c], mask=coeff[i, :c], score=score[i, :c], proto=proto[i],
                                           prior=prior[i, :c], **{"class": cls[i, :c]})
            out.append({"detection": det, "net": self, "_index": i, "_forward": self._forward_id})
            if total is not None:  # survivors of the suppression pass before the cut to max_num_detections (cross-class / traditional NMS)
                out[-1]["nms_total"] = int(total[i])
        return out

    def check_nms_overflow(self, n):
        """After a synchronised forward in nms_mode 1 / 2: det.nms_total [n], or NmsCapOverflow if the traditional mode's per-class capacity
        may have changed an image's result (det.nms_overflow).  None in the default mode, which has neither buffer."""
        if not self.nms_mode:
            return None
        over = self.fetch("det.nms_overflow", n)
        if over.any():
            raise NmsCapOverflow("traditional NMS: a class of image(s) %s holds more than nms_trad_cap = %d candidates and fewer than "
                                 "max_num_detections of those survived; raise nms_trad_cap (at most 2048)"
                                 % (np.nonzero(over)[0].tolist(), self.nms_trad_cap))
        return self.fetch("det.nms_total", n)


def postprocess(det_output, w, h, batch_idx=0, score_threshold=0.0):
    """Yolact layers/output_utils.postprocess (Y7): (classes, scores, boxes[int64 xyxy], masks[n,h,w] uint8).

    Masks are produced on the GPU for the whole last batch at (h, w); `score_threshold` filters the
    (score-sorted) detections afterwards, which is equivalent because the filter precedes all
    arithmetic upstream and every detection's mask is independent."""
    dets = det_output[batch_idx]
    net = dets["net"]
    if dets["detection"] is None:
        z = np.zeros((0,), np.int32)
        return z, np.zeros((0,), np.float32), np.zeros((0, 4), np.int64), np.zeros((0, h, w), np.uint8)
    i = dets["_index"]
    if dets.get("_forward", net._forward_id) != net._forward_id:
        raise RuntimeError("postprocess(): these predictions come from an earlier forward of this net; the device buffers "
                           "(prototypes, coefficients) now hold a later batch")
    key = (h, w, net._forward_id)
    if getattr(net, "_pp_key", None) != key:
        net.postprocess_device(h, w)
        net.sync()
        net._pp_key = key
        net._pp_masks = net.fetch("det.masks")
        net._pp_boxes = net.fetch("det.box_int")
        net._pp_mask_scores = net.fetch("det.mask_score") if net.has_maskiou else None
    d = dets["detection"]
    keep = d["score"] > np.float32(score_threshold)
    c = len(d["score"])
    scores = d["score"][keep]
    if net.has_maskiou:  # upstream (rescore_mask, not rescore_bbox): scores = [box scores, box scores * mask IoU]
        scores = [scores, net._pp_mask_scores[i, :c][keep]]
    return d["class"][keep], scores, net._pp_boxes[i, :c][keep], net._pp_masks[i, :c][keep]


def render_images(net, images, score_threshold=0.0, top_k=None, batch_size=None):
    """eval.py --image / --images with the drawing on the device: -> one annotated HxWx3 uint8 BGR array per image, bit-identical to
    cli._overlay(image, masks, boxes, classes) of postprocess(net(batch), w, h, i, score_threshold) cut to its first top_k detections.
    Per batch: the uint8 front end, the forward, then per image postprocess_device at the image's own (h, w) and isegmi_engine_paint over its rows of
    det.masks.  The detection arrays (count, score, class, integer boxes) come back; the mask planes never leave the device."""
    from .render import yolact_entries
    images = [np.ascontiguousarray(im, np.uint8) for im in images]
    bs = int(batch_size or net.max_batch)
    assert 0 < bs <= net.max_batch
    out = []
    for j in range(0, len(images), bs):
        batch = images[j:j + bs]
        n = net.upload_u8(batch)
        net.forward_device(n)
        net.sync()
        net.check_nms_overflow(n)
        cnt, score, cls = net.fetch("det.count", n), net.fetch("det.score", n), net.fetch("det.class", n)
        for i, im in enumerate(batch):
            h, w = im.shape[:2]
            c = int(cnt[i])
            keep = np.nonzero(score[i, :c] > np.float32(score_threshold))[0]
            if top_k is not None:
                keep = keep[:top_k]
            if not len(keep):
                out.append(im.copy())
                continue
            net.postprocess_device(h, w)   # the whole batch at this image's size, as postprocess() does: rows of image i are the planes it returns
            net.sync()
            boxes = net.fetch("det.box_int", n)[i]
            out.append(net.paint_device(im, yolact_entries(keep, boxes[keep], cls[i, keep], h, w), index=i))
    return out


def evaluate(net, images, image_ids=None, batch_size=None, score_threshold=0.0, top_k=None, rank=0, world=1, sizes=None, stats=None, force_gather=False):
    """eval.py's image evaluation as a data-set loop (README.md:243-249: --images / --output_coco_json): images -> COCO-format result list
    (Detections.add_bbox / add_mask records) -- the path the benchmark measures, end to end.  Batches of `batch_size` raw uint8 BGR
    images (any sizes) go up through pinned memory; FastBaseTransform, the forward, Detect, postprocess at every image's OWN size,
    pycocotools RLE and the packing of one fixed-size record block run on the device; the block comes back asynchronously (one rank) or
    is all-gathered over RCCL (`world` ranks, batches round-robin) while the next batch computes.

    images: sequence of HxWx3 uint8 BGR arrays, or a callable i -> array together with sizes = [(h, w), ...]."""
    import time
    from .coco import results_from_records
    from .pipeline import record_capacity, run_record_loop
    get = images if callable(images) else images.__getitem__
    if sizes is None:
        if callable(images):
            raise ValueError("evaluate(): a callable image source needs sizes=[(h, w), ...]")
        sizes = [im.shape[:2] for im in images]
    n_img = len(sizes)
    ids = list(image_ids) if image_ids is not None else list(range(n_img))
    bs = int(batch_size or net.max_batch)
    assert bs <= net.max_batch
    batches = [list(range(j, min(j + bs, n_img))) for j in range(0, n_img, bs)]
    K = record_capacity(net)
    pin_bytes = max(sum(sizes[i][0] * sizes[i][1] * 3 for i in b) for b in batches) if batches else 1
    pin = [_ffi.PinnedBuffer((pin_bytes,), np.uint8) for _ in range(2)]
    for slot in (0, 1):
        net._u8_staging(slot, pin_bytes)   # both device staging buffers at their final size: no sync + re-allocation when a later batch is larger
    per_image = [None] * n_img

    def consume(step, recs):
        for r, rec in enumerate(recs):
            j = step * world + r
            if j >= len(batches):
                continue
            b = batches[j]
            res = results_from_records(rec, [ids[i] for i in b] + [None] * (bs - len(b)), [sizes[i] for i in b] + [(1, 1)] * (bs - len(b)), 1,
                                       K, score_threshold, top_k)
            by_id = {}
            for d in res:
                by_id.setdefault(d["image_id"], []).append(d)
            for i in b:
                per_image[i] = by_id.get(ids[i], [])

    def enqueue(step, slot):
        j = step * world + rank
        if j >= len(batches):
            return False
        b = batches[j]
        off = 0
        for i in b:
            im = np.ascontiguousarray(get(i), np.uint8)
            pin[slot].array[off:off + im.size] = im.reshape(-1)
            off += im.size
        hw = [sizes[i] for i in b]
        net.upload_u8_async(pin[slot], len(b), slot=slot, sizes_hw=hw)
        net.forward_device(len(b), slot)
        net.postprocess_device_sizes(hw)
        net.rle_device(hw)
        return True

    t0 = time.perf_counter()
    nsteps = -(-len(batches) // world)
    try:
        run_record_loop(net, bs, nsteps, enqueue, consume, rank, world, force_gather)   # closes its pipeline / gather on every way out
    finally:
        for p in pin:
            p.free()
    if stats is not None:
        stats.update(steps=nsteps, images=n_img, seconds=time.perf_counter() - t0, batches=len(batches), batch_size=bs, world=world)
    return [d for r in per_image if r for d in r]
