"""YOLOv3 inference, host side ([UPSTREAM-RECALL] the public yolov3.cfg / COCO-80 model, unverified: the reference's yolo.jittor directory is
empty).  `net = YoloV3(sd, H, W)`; `dets = net(batch)` -> per image boxes (canvas coordinates), scores, labels 1..C.  `YoloDetector(...).detect(images)`
adds the letterbox front end and maps the boxes back to the original images.  All numerics run in libisegmi.so (engine kind 5); this module moves
config, weights and results across the C ABI.  The letterbox runs on the host by default (PIL); YoloDetector(..., resize="device") uploads the original
bytes and runs it on the device (isegmi_engine_resample_u8: PIL-exact resize, x / 255, RGB, 0.5 border), bit-identical.
YoloV3Config.variant selects yolov3, yolov3-spp or yolov3-tiny; pool_pad is the pad switch of the two variants' max-pools."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .engine import DetectionBlock, Engine
from .weights import YOLO_VARIANTS, fold_batchnorm, to_krsc, yolo_layers

YOLO_MAX_TOP_N = 1024    # csrc/yolo_ops.hip YOLO_KCAP
YOLO_MAX_CLASSES = 255   # the class-wise NMS holds 256 labels with the background
YOLO_STRIDES = (32, 16, 8)
YOLO_ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
YOLO_MASKS = ((6, 7, 8), (3, 4, 5), (0, 1, 2))
YOLO_TINY_ANCHORS = ((10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319))
YOLO_TINY_MASKS = ((3, 4, 5), (0, 1, 2))   # this project's yolov3-tiny.cfg; pjreddie's original has 1,2,3 in the second


@dataclass(frozen=True)
class YoloV3Config:
    """yolov3.cfg inference constants.  anchors: the cfg's nine (w, h) pairs in pixels; masks: the anchors of the [yolo] layers in file order (stride 32
    first).  multi_label True: every class with objectness x class > conf_thresh is a candidate (darknet, ultralytics); False: the best class only
    (the PyTorch-YOLOv3 ports).  bn_eps: 1e-5 (the PyTorch ports); darknet's own normaliser uses 1e-6.  variant: "yolov3", "spp"
    (yolov3-spp.cfg) or "tiny" (yolov3-tiny.cfg: two [yolo] layers, strides 32 and 16; YoloV3Config.tiny() has its anchors and masks).  pool_pad: what a
    tap outside the map is to the variants' max-pools -- "ignore" (darknet: skipped) or "zero" (the PyTorch ports' ZeroPad2d + MaxPool2d: a 0)."""
    height: int = 416
    width: int = 416
    classes: int = 80
    anchors: tuple = YOLO_ANCHORS
    masks: tuple = YOLO_MASKS
    conf_thresh: float = 0.5
    nms_thresh: float = 0.4
    pre_nms_top_n: int = 1024
    multi_label: bool = True
    min_wh: float = 0.0
    detections_per_img: int = 100
    detections_cap: int = 0
    nms_ge: int = 0
    nms_plus_one: int = 0          # plain areas
    nms_output_order: str = "score"
    bn_eps: float = 1e-5
    variant: str = "yolov3"
    pool_pad: str = "ignore"

    @classmethod
    def tiny(cls, **kw):
        return cls(**dict(dict(variant="tiny", anchors=YOLO_TINY_ANCHORS, masks=YOLO_TINY_MASKS), **kw))

    @property
    def det_cap(self):
        return max(self.detections_per_img, self.detections_cap)

    @property
    def strides(self):
        """The strides of the [yolo] layers in file order."""
        return YOLO_STRIDES[:2] if self.variant == "tiny" else YOLO_STRIDES

    def level_anchors(self):
        """[levels][3][2] float32: the anchors of head s (s = 0 at stride 32)."""
        return np.asarray([[self.anchors[i] for i in m] for m in self.masks], np.float32)

    def validate(self, H=None, W=None):
        """Raises ValueError naming the key that is refused."""
        for key, v in (("height", self.height if H is None else H), ("width", self.width if W is None else W)):
            if v % 32 or not 32 <= v <= 1024:
                raise ValueError("%s=%d: canvas sides are multiples of 32 in 32..1024" % (key, v))
        if not 1 <= self.classes <= YOLO_MAX_CLASSES:
            raise ValueError("classes=%d: 1..%d classes are built" % (self.classes, YOLO_MAX_CLASSES))
        if self.variant not in YOLO_VARIANTS:
            raise ValueError("variant=%r: yolov3, spp or tiny" % (self.variant,))
        if self.pool_pad not in ("ignore", "zero"):
            raise ValueError("pool_pad=%r: ignore or zero" % (self.pool_pad,))
        if len(self.masks) != len(self.strides) or any(len(m) != 3 for m in self.masks):
            raise ValueError("masks=%r: %s [yolo] layers of three anchors each are built (A = 3) for variant %s"
                             % (self.masks, "two" if self.variant == "tiny" else "three", self.variant))
        if any(not 0 <= i < len(self.anchors) for m in self.masks for i in m) or any(len(a) != 2 or a[0] <= 0 or a[1] <= 0 for a in self.anchors):
            raise ValueError("anchors=%r: positive (w, h) pairs, every mask index inside the list" % (self.anchors,))
        if not 1 <= self.pre_nms_top_n <= YOLO_MAX_TOP_N:
            raise ValueError("pre_nms_top_n=%d: the selection kernels hold 1..%d per level" % (self.pre_nms_top_n, YOLO_MAX_TOP_N))
        if not self.conf_thresh >= 0:
            raise ValueError("conf_thresh=%r: a non-negative number" % (self.conf_thresh,))
        if not self.nms_thresh > 0:
            raise ValueError("nms_thresh=%r: a positive number" % (self.nms_thresh,))
        if not self.min_wh >= 0:
            raise ValueError("min_wh=%r: a non-negative number" % (self.min_wh,))
        if self.nms_output_order not in ("score", "index"):
            raise ValueError("nms_output_order=%r: score or index" % (self.nms_output_order,))
        return self


def yolo_grids(H, W, strides=YOLO_STRIDES):
    """(h, w) of the heads' grids on an (H, W) canvas, stride 32 first."""
    return [(H // s, W // s) for s in strides]


def yolov3_folded(sd, cfg=YoloV3Config()):
    """{layer: (weight [Cout][R][S][Cin], scale or None, shift)}: BN folded with cfg.bn_eps, the predictors with their bias."""
    out = {}
    for name, bn, cout, cin, k in yolo_layers(cfg.variant, cfg.classes):
        w = np.asarray(sd[name + ".weight"], np.float32)
        if w.shape != (cout, cin, k, k):
            raise ValueError("%s.weight: expected %s, got %s" % (name, (cout, cin, k, k), w.shape))
        sc, sh = fold_batchnorm(sd, bn, cfg.bn_eps) if bn else (None, np.asarray(sd[name + ".bias"], np.float32))
        out[name] = (to_krsc(w), sc, sh)
    return out


class YoloV3(Engine, DetectionBlock):
    KIND = 5

    def __init__(self, state_dict, H=None, W=None, cfg=YoloV3Config(), max_batch=8, device=0, fp16=False, graph=False):
        if fp16:
            raise ValueError("YoloV3: fp16=True is not built (fp32 only)")
        if graph:
            raise ValueError("YoloV3: graph=True (hipGraph capture) is not built")
        H, W = int(cfg.height if H is None else H), int(cfg.width if W is None else W)
        cfg.validate(H, W)
        self.cfg, self.H, self.W, self.max_batch = cfg, H, W, max_batch
        self.fp16 = False
        self._create(device, max_batch, H, W)
        for name, (w, sc, sh) in yolov3_folded(state_dict, cfg).items():
            if w.shape[3] % 32:   # the 3-channel image, and tiny's 16-channel first map, run as zero-padded 32-channel copies
                w = np.concatenate([w, np.zeros(w.shape[:3] + (32 - w.shape[3],), np.float32)], -1)
            if cfg.variant == "tiny" and name == "backbone.conv0":   # 16 -> 32 rows: output channels 16..31 are zero weights with scale 1 and shift 0 -> LeakyReLU(0) = 0
                w = np.concatenate([w, np.zeros((16,) + w.shape[1:], np.float32)], 0)
                sc, sh = np.concatenate([sc, np.ones(16, np.float32)]), np.concatenate([sh, np.zeros(16, np.float32)])
            self._set_conv_krsc(name, w, sc, sh)
        self.set_param("yolo_variant", float(YOLO_VARIANTS.index(cfg.variant)))
        for i, v in enumerate(cfg.level_anchors().reshape(-1)):
            self.set_param("yolo_anchor%d" % i, float(v))
        self.configure(cfg)
        self._d_in = _ffi.DeviceBuffer((max_batch, H, W, 3))

    def configure(self, cfg):
        """The tail's parameters from a config (live: the next forward uses them)."""
        cfg.validate(self.H, self.W)
        if cfg.variant != self.cfg.variant:
            raise ValueError("variant=%r: the engine was built as %r (the graph and its weights are fixed at construction)" % (cfg.variant, self.cfg.variant))
        for k, v in (("yolo_pool_zero_pad", cfg.pool_pad == "zero"), ("yolo_conf_thresh", cfg.conf_thresh), ("yolo_nms_thresh", cfg.nms_thresh), ("yolo_pre_nms_top_n", cfg.pre_nms_top_n),
                     ("yolo_multi_label", float(bool(cfg.multi_label))), ("yolo_min_wh", cfg.min_wh), ("detections_per_img", cfg.detections_per_img),
                     ("detections_cap", cfg.detections_cap), ("nms_ge", cfg.nms_ge), ("nms_plus_one", cfg.nms_plus_one),
                     ("nms_index_order", {"score": 0, "index": 1}[cfg.nms_output_order])):
            self.set_param(k, float(v))
        self.cfg = cfg

    def rle_device(self, image_hw=None):
        raise RuntimeError("rle_device: YoloV3 is a box detector: there are no masks to encode")

    def upload(self, batch_nhwc3, slot=0):
        """A letterboxed fp32 batch [n, H, W, 3] (RGB, x / 255)."""
        x = np.ascontiguousarray(batch_nhwc3, np.float32)
        assert x.ndim == 4 and x.shape[1:] == (self.H, self.W, 3) and x.shape[0] <= self.max_batch, x.shape
        _ffi.check(_ffi.lib().isegmi_h2d(self.input_buffer(slot).ptr, x.ctypes.data_as(C.c_void_p), x.nbytes))
        return x.shape[0]

    def upload_original_u8(self, images_bgr_u8, slot=0):
        """The letterbox on the device: ORIGINAL HxWx3 uint8 BGR images -> the canvas batch yolo_letterbox makes on the host, bit for bit:
        one upload of the bytes and their tables, one launch (resize to the letterbox size at (pad_y, pad_x), x / 255, RGB, 0.5 elsewhere).
        -> (n, [(gain, pad_x, pad_y)])"""
        from .transforms import ResamplePlan, letterbox_geometry
        ims = [np.ascontiguousarray(im) for im in images_bgr_u8]
        assert 0 < len(ims) <= self.max_batch
        if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in ims):
            raise TypeError("upload_original_u8 takes HxWx3 uint8 images")
        geo = [letterbox_geometry(im.shape[0], im.shape[1], self.H, self.W) for im in ims]
        plan = ResamplePlan([im.shape[:2] for im in ims], [[(i, nh, nw, py, px, 0, i) for i, (_, nh, nw, px, py) in enumerate(geo)]])
        flat = np.empty(plan.nbytes, np.uint8)
        plan.write(flat, ims)
        st = self._u8_staging(slot, plan.nbytes)
        _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, flat.ctypes.data_as(C.c_void_p), plan.nbytes))
        self._resample_u8(st, plan, 0, self.input_buffer(slot).ptr.value, len(ims), self.H, self.W, (0.0, 0.0, 0.0), (255.0, 255.0, 255.0), True, 0.5)
        return len(ims), [(g, px, py) for g, _, _, px, py in geo]

    def forward_device(self, n, slot=0):
        _ffi.check(_ffi.lib().isegmi_yolov3_forward(self._h, self.input_buffer(slot).ptr, n))

    def detections(self, n):
        cnt, box, score, label = (self.fetch(k, n) for k in ("det.count", "det.box", "det.score", "det.label"))
        return [dict(box=box[i, :cnt[i]].copy(), score=score[i, :cnt[i]].copy(), label=label[i, :cnt[i]].copy()) for i in range(n)]

    def __call__(self, batch_nhwc3):
        """-> per image dict(box [k, 4] xyxy in canvas coordinates, score [k], label [k] in 1..classes)."""
        n = self.upload(batch_nhwc3)
        self.forward_device(n)
        self.sync()
        return self.detections(n)

    def heads(self, n):
        """The raw head tensors of the last forward, stride 32 first: [n, H_s, W_s, 3 * (5 + classes)]."""
        return [self.fetch("yolo.head%d" % s, n) for s in range(len(self.cfg.strides))]

    def candidate_counts(self, n):
        """(kept [n, levels], before the top-n cut [n, levels]) per (image, level) of the last forward: kept < before means the cut truncated that level."""
        return self.fetch("yolo.cand_cnt", n), self.fetch("yolo.cand_total", n)


class YoloDetector:
    """Images in, detections in original image coordinates out: letterbox on the host (resize="host", PIL) or on the device (resize="device": the original
    bytes go up, YoloV3.upload_original_u8), YoloV3 on the device, the back mapping in numpy fp32.  Both modes give identical detections."""

    def __init__(self, state_dict, cfg=YoloV3Config(), max_batch=8, device=0, resize="host"):
        if resize not in ("host", "device"):
            raise ValueError("resize: 'host' (PIL letterbox) or 'device' (isegmi_engine_resample_u8; DESIGN.md 24)")
        self.cfg, self.resize = cfg, resize
        self.net = YoloV3(state_dict, cfg.height, cfg.width, cfg, max_batch=max_batch, device=device)

    def detect(self, images_bgr_u8):
        """list of HxWx3 uint8 BGR images -> list of (boxes [k, 4] xyxy float32, scores [k], labels [k])."""
        from .transforms import yolo_letterbox, yolo_unletterbox
        out = []
        B = self.net.max_batch
        for i0 in range(0, len(images_bgr_u8), B):
            ims = images_bgr_u8[i0:i0 + B]
            if self.resize == "device":
                n, geos = self.net.upload_original_u8(ims)
                self.net.forward_device(n)
                self.net.sync()
                for im, geo, d in zip(ims, geos, self.net.detections(n)):
                    out.append((yolo_unletterbox(d["box"], geo, im.shape[0], im.shape[1]), d["score"], d["label"]))
                continue
            lb = [yolo_letterbox(im, self.cfg.height, self.cfg.width) for im in ims]
            dets = self.net(np.stack([x for x, _ in lb]))
            for im, (_, geo), d in zip(ims, lb, dets):
                out.append((yolo_unletterbox(d["box"], geo, im.shape[0], im.shape[1]), d["score"], d["label"]))
        return out

    def close(self):
        self.net.close()
