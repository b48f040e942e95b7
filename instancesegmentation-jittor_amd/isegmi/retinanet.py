"""RetinaNet R-50/R-101-FPN inference, host side ([UPSTREAM-RECALL] maskrcnn-benchmark retinanet/retinanet_R-50-FPN_1x.yaml, the one-stage
detector of the config tree detectron.jittor ports, README.md:252-347).  `model = RetinaNet(sd, H, W)`; `preds = model(batch, image_hw)` -> one BoxList per
image with scores and labels.  All numerics run in libisegmi.so (engine kind 4); this module moves config, weights, anchors and results across the C ABI.
The calling surface is MaskRCNN's: one engine serves every canvas up to (H, W), uploads go through the same device front end."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .engine import DetectionBlock
from .maskrcnn import BoxList, MaskRCNN, generate_anchors_multi, resnext_refusals
from .weights import fold_frozen_batchnorm, to_krsc

RETINA_MAX_TOP_N = 1024   # csrc/retinanet_ops.hip RETINA_KCAP
RETINA_LEVELS = 5


@dataclass(frozen=True)
class RetinaNetConfig:
    """retinanet_R-50-FPN_1x inference constants; key names follow the yaml (MODEL.RETINANET.*, TEST.DETECTIONS_PER_IMG)."""
    depth: int = 50
    CONV_BODY: str = "R-50-FPN-RETINANET"
    MIN_SIZE_TEST: int = 800
    MAX_SIZE_TEST: int = 1333
    SIZE_DIVISIBILITY: int = 32
    NUM_CLASSES: int = 81
    ANCHOR_SIZES: tuple = (32, 64, 128, 256, 512)
    ANCHOR_STRIDES: tuple = (8, 16, 32, 64, 128)
    ASPECT_RATIOS: tuple = (0.5, 1.0, 2.0)
    OCTAVE: float = 2.0
    SCALES_PER_OCTAVE: int = 3
    NUM_CONVS: int = 4
    PRE_NMS_TOP_N: int = 1000
    INFERENCE_TH: float = 0.05
    NMS_TH: float = 0.4
    DETECTIONS_PER_IMG: int = 100
    DETECTIONS_CAP: int = 0          # rows per image in the detection buffers: 0 = DETECTIONS_PER_IMG; more receives the ties at the cut
    NMS_GE: int = 0                  # the NMS forks of MaskRCNNConfig, applied to the class-wise NMS
    NMS_PLUS_ONE: int = 1
    NMS_OUTPUT_ORDER: str = "score"
    FROZEN_BN_EPS: float = 0.0
    STRIDE_IN_1X1: bool = True
    NUM_GROUPS: int = 1          # MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP: the ResNeXt trunk (retinanet_X_101_32x8d_FPN_1x), as MaskRCNNConfig
    WIDTH_PER_GROUP: int = 64

    @property
    def det_cap(self):
        return max(self.DETECTIONS_PER_IMG, self.DETECTIONS_CAP)

    @property
    def is_c4(self):
        return False

    def level_sizes(self, size):
        """Anchor sizes of one level: size * OCTAVE ** (s / SCALES_PER_OCTAVE), in Python floats."""
        return tuple(size * self.OCTAVE ** (s / float(self.SCALES_PER_OCTAVE)) for s in range(self.SCALES_PER_OCTAVE))


def retina_level_shapes(H, W):
    """(h, w) of P3..P7 on an (H, W) canvas: P3 = canvas / 8, then five halvings rounded up (3x3 stride 2 pad 1)."""
    s = (H // 8, W // 8)
    out = [s]
    for _ in range(4):
        s = ((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1)
        out.append(s)
    return out


class RetinaNet(MaskRCNN, DetectionBlock):
    KIND = 4

    def __init__(self, state_dict, H, W, cfg=RetinaNetConfig(), max_batch=2, device=0, fp16=False, graph=False):
        if fp16:
            raise ValueError("RetinaNet: fp16=True is not built (fp32 only)")
        resnext_refusals(cfg, fp16)
        if graph:
            raise ValueError("RetinaNet: graph=True (hipGraph capture) is not built")
        if len(cfg.ANCHOR_STRIDES) != RETINA_LEVELS or len(cfg.ANCHOR_SIZES) != RETINA_LEVELS:
            raise ValueError("MODEL.RETINANET.ANCHOR_STRIDES / ANCHOR_SIZES: five levels (P3-P7) are built, got %d / %d" % (len(cfg.ANCHOR_STRIDES), len(cfg.ANCHOR_SIZES)))
        if not 1 <= cfg.PRE_NMS_TOP_N <= RETINA_MAX_TOP_N:
            raise ValueError("MODEL.RETINANET.PRE_NMS_TOP_N=%d: the selection kernels hold 1..%d per level" % (cfg.PRE_NMS_TOP_N, RETINA_MAX_TOP_N))
        if cfg.NUM_CONVS < 1:
            raise ValueError("MODEL.RETINANET.NUM_CONVS=%d: at least one tower convolution" % cfg.NUM_CONVS)
        assert H % cfg.SIZE_DIVISIBILITY == 0 and W % cfg.SIZE_DIVISIBILITY == 0 and cfg.SIZE_DIVISIBILITY % 32 == 0
        self.cfg, self.H, self.W, self.max_batch = cfg, H, W, max_batch
        self.fp16 = False
        self.mask_buf = None
        self._create(device, max_batch, H, W)
        self._load(state_dict)
        for k, v in (("resnet_depth", cfg.depth), ("stride_in_1x1", float(bool(cfg.STRIDE_IN_1X1))), ("retina_pre_nms_top_n", cfg.PRE_NMS_TOP_N),
                     ("retina_inference_th", cfg.INFERENCE_TH), ("retina_nms_th", cfg.NMS_TH), ("retina_num_convs", cfg.NUM_CONVS),
                     ("retina_levels", len(cfg.ANCHOR_STRIDES)), ("detections_per_img", cfg.DETECTIONS_PER_IMG), ("detections_cap", cfg.DETECTIONS_CAP),
                     ("nms_ge", cfg.NMS_GE), ("nms_plus_one", cfg.NMS_PLUS_ONE), ("nms_index_order", {"score": 0, "index": 1}[cfg.NMS_OUTPUT_ORDER])):
            self.set_param(k, float(v))
        self._d_in = _ffi.DeviceBuffer((max_batch, H, W, 3))
        self._hw = None
        self._canvas = (H, W)

    def _load(self, sd):
        cfg = self.cfg
        w = to_krsc(sd["backbone.body.stem.conv1.weight"])
        w = np.concatenate([w, np.zeros(w.shape[:3] + (1,), np.float32)], -1)
        self._set_conv_krsc("backbone.body.stem.conv1", w, *fold_frozen_batchnorm(sd, "backbone.body.stem.bn1", cfg.FROZEN_BN_EPS))
        for li, nb in enumerate((3, 4, 23 if cfg.depth == 101 else 6, 3), 1):
            self._load_bottlenecks(sd, "backbone.body.layer%d" % li, "backbone.body.layer%d" % li, nb, stage=li - 1)
        names = ["backbone.fpn.fpn_%s%d" % (k, i) for i in (2, 3, 4) for k in ("inner", "layer")] + ["backbone.fpn.top_blocks.p6", "backbone.fpn.top_blocks.p7"]
        names += ["rpn.head.%s_tower.%d" % (t, 2 * i) for i in range(cfg.NUM_CONVS) for t in ("cls", "bbox")] + ["rpn.head.cls_logits", "rpn.head.bbox_pred"]
        for nm in names:
            self._set_conv_krsc(nm, to_krsc(sd[nm + ".weight"]), None, sd[nm + ".bias"])
        if "rpn.head.cls_tower.%d.weight" % (2 * cfg.NUM_CONVS) in sd:
            raise ValueError("rpn.head.cls_tower: more layers in the weights than MODEL.RETINANET.NUM_CONVS=%d" % cfg.NUM_CONVS)
        A = len(cfg.ASPECT_RATIOS) * cfg.SCALES_PER_OCTAVE
        if sd["rpn.head.cls_logits.weight"].shape[0] != A * (cfg.NUM_CLASSES - 1) or sd["rpn.head.bbox_pred.weight"].shape[0] != A * 4:
            raise ValueError("rpn.head.cls_logits / bbox_pred: expected %d x %d and %d x 4 output channels" % (A, cfg.NUM_CLASSES - 1, A))
        for l, (stride, size) in enumerate(zip(cfg.ANCHOR_STRIDES, cfg.ANCHOR_SIZES)):
            self._set_tensor("anchor_base.%d" % l, generate_anchors_multi(stride, cfg.level_sizes(size), cfg.ASPECT_RATIOS))
            self.set_param("anchor_stride%d" % l, float(stride))

    def reserve(self):
        """Size every buffer for the largest canvas and batch with one forward on a zero batch.  Returns memory()."""
        self._d_in.zero()
        self._hw = np.tile(np.array([[self.H, self.W]], np.int32), (self.max_batch, 1))
        self._canvas = (self.H, self.W)
        self.forward_device(self.max_batch)
        self.sync()
        return self.memory()

    def forward_device(self, n, slot=0):
        H, W = self._canvas
        _ffi.check(_ffi.lib().isegmi_retinanet_forward_canvas(self._h, self.input_buffer(slot).ptr, self._hw.ctypes.data_as(C.c_void_p), n, H, W))

    def paste_device(self, *a, **k):
        raise _ffi.IsegmiError("RetinaNet has no masks to paste")

    def boxlists(self, n, cnt, box, score, label):
        out = []
        for i in range(n):
            c = int(cnt[i])
            bl = BoxList(box[i, :c], (int(self._hw[i, 1]), int(self._hw[i, 0])))
            bl.add_field("scores", score[i, :c].copy()); bl.add_field("labels", label[i, :c].astype(np.int64))
            out.append(bl)
        return out

    def __call__(self, batch_nhwc3, image_hw=None):
        """-> list of BoxList (one per image, network-input coordinates) with scores and labels 1..80.  image_hw None: a list of already-resized uint8
        BGR images through the device front end."""
        return self._detect(self.upload_u8(batch_nhwc3) if image_hw is None else self.upload(batch_nhwc3, image_hw))

    def _detect(self, n):
        self.forward_device(n)
        self.sync()
        return self.boxlists(n, *(self.fetch(k, n) for k in ("det.count", "det.box", "det.score", "det.label")))

    def selected(self, n):
        """Every level's selected list of the last forward: [l][i] = (scores, flat indices)."""
        cnt, s, idx = (self.fetch(k, n) for k in ("retina.sel_cnt", "retina.sel_score", "retina.sel_idx"))
        return [[(s[i, l, : cnt[i, l]], idx[i, l, : cnt[i, l]]) for i in range(n)] for l in range(RETINA_LEVELS)]
