"""Mask R-CNN R50/R101-FPN inference, host side (mirrors detectron.jittor's predictor surface).

Reference surface (README.md:288-335): `cfg.merge_from_file(...)`; `COCODemo(cfg, min_image_size=800,
confidence_threshold=0.5)`; `coco_demo.run_on_opencv_image(image)`; [UPSTREAM-RECALL, SURVEY 8b]
`compute_prediction(image) -> BoxList` with fields scores / labels / mask.  All numerics run in
libisegmi.so; this module moves config, weights, anchors and results across the C ABI.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _ffi
from .engine import Engine
from .weights import fold_frozen_batchnorm, to_krsc

PIXEL_MEAN = (102.9801, 115.9465, 122.7717)  # BGR, TO_BGR255


@dataclass(frozen=True)
class MaskRCNNConfig:
    """e2e_mask_rcnn_R_50_FPN_1x inference constants; key names follow the yaml."""
    depth: int = 50
    MIN_SIZE_TEST: int = 800
    MAX_SIZE_TEST: int = 1333
    SIZE_DIVISIBILITY: int = 32
    ANCHOR_SIZES: tuple = (32, 64, 128, 256, 512)
    ANCHOR_STRIDE: tuple = (4, 8, 16, 32, 64)
    ASPECT_RATIOS: tuple = (0.5, 1.0, 2.0)
    RPN_PRE_NMS_TOP_N_TEST: int = 1000
    RPN_POST_NMS_TOP_N_TEST: int = 1000
    RPN_FPN_POST_NMS_TOP_N_TEST: int = 1000
    RPN_NMS_THRESH: float = 0.7
    RPN_MIN_SIZE: float = 0.0
    ROI_SCORE_THRESH: float = 0.05
    ROI_NMS: float = 0.5
    DETECTIONS_PER_IMG: int = 100
    DETECTIONS_CAP: int = 0  # rows per image in the detection buffers; 0 = DETECTIONS_PER_IMG.  upstream's kth-value cut keeps every detection that
    #                          TIES with the 100th score, so an image can return more than DETECTIONS_PER_IMG: set e.g. 128 to receive those ties
    #                          (the mask head then runs over that many RoI slots per image); with 0 ties past the 100th row are cut in output order
    # Semantic forks: which side detectron.jittor takes cannot be checked (the reference tree holds no code), so each
    # is a switch, mirrored in the oracle (oracle/maskrcnn_ref.py) and run through the engine by tests/test_forks_gpu.py.  Defaults = maskrcnn-benchmark's
    # CUDA path.
    NMS_GE: int = 0             # 0 suppress on iou > thr (CUDA kernel, jt.nms), 1 on >= (CPU loop)
    NMS_PLUS_ONE: int = 1       # 1 legacy +1 widths in the NMS IoU (RPN and box post-processing), 0 plain areas
    NMS_OUTPUT_ORDER: str = "score"   # order of a class's detections after the box NMS: "score" (CUDA kernel) or "index" (CPU: nonzero(keep), proposal order)
    ROI_ALIGNED: int = 0        # 0 legacy ROIAlign (no half-pixel shift, RoI >= 1 pixel), 1 ROIAlign(aligned=True)
    FROZEN_BN_EPS: float = 0.0  # FrozenBatchNorm2d: scale = w * rsqrt(var + eps); maskrcnn-benchmark has no eps
    # Opt-in NUMERICS MODE for latency (not a semantic fork: the same sums in another fp32 association): the backbone's small-M / large-K bottleneck
    # convolutions (a bs = 1 forward) as four k-ordered partial chains added left to right -- conv tile 15, include/isegmi.h; bit-exact against the oracle
    # model run with conv_split_k=1, NOT against the default mode; results then depend on the batch size a layer is run at (the rule is by shape)
    CONV_SPLIT_K: int = 0
    CONV_BODY: str = "R-50-FPN"  # "R-50-FPN" / "R-101-FPN" (depth) or "R-50-C4" (the yaml README.md:263-273 prints)
    # [UPSTREAM-RECALL] gn_baselines: GroupNorm in the backbone (StemWithGN / BottleneckWithGN), the FPN, the Xconv1fc box head and the
    # mask head -- all of them or none (config.to_maskrcnn_config refuses the mixtures).  fp32 only.
    USE_GN: bool = False
    GN_NUM_GROUPS: int = 32      # MODEL.GROUP_NORM.NUM_GROUPS
    GN_DIM_PER_GP: int = -1      # MODEL.GROUP_NORM.DIM_PER_GP: > 0 -> groups = C / DIM_PER_GP (then NUM_GROUPS is unused)
    GN_EPSILON: float = 1e-5     # MODEL.GROUP_NORM.EPSILON
    STRIDE_IN_1X1: bool = True   # MODEL.RESNETS.STRIDE_IN_1X1: a stage's stride on conv1 (True) or on the 3x3 (False: the GN yaml)
    BOX_HEAD: str = "FPN2MLPFeatureExtractor"   # or "FPNXconv1fcFeatureExtractor" (with USE_GN)
    BOX_HEAD_STACKED_CONVS: int = 4   # MODEL.ROI_BOX_HEAD.NUM_STACKED_CONVS
    BOX_HEAD_CONV_DIM: int = 256      # MODEL.ROI_BOX_HEAD.CONV_HEAD_DIM
    BOX_HEAD_MLP_DIM: int = 1024      # MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM
    # [UPSTREAM-RECALL] DESIGN.md 13.  MASK_ON False = Faster R-CNN (e2e_faster_rcnn_*): roi_heads = [box] only, results are boxes, scores and labels.
    # Upstream's default is False; this project's stays True (the yamls under configs/ spell the key out).
    MASK_ON: bool = True
    NUM_CLASSES: int = 81                  # MODEL.ROI_BOX_HEAD.NUM_CLASSES, background included (2..257)
    CLS_AGNOSTIC_BBOX_REG: bool = False    # MODEL.CLS_AGNOSTIC_BBOX_REG: bbox_pred has 2 * 4 outputs, the last four decoded once per proposal
    # [UPSTREAM-RECALL] DESIGN.md 14.  KEYPOINT_ON = Keypoint R-CNN (e2e_keypoint_rcnn_*): roi_heads = [box, keypoint]; MASK_ON False, FrozenBN FPN body, fp32.
    KEYPOINT_ON: bool = False
    KEYPOINT_CONV_LAYERS: tuple = (512,) * 8   # MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS: widths of conv_fcn1.. (multiples of 32)
    NUM_KEYPOINTS: int = 17                    # MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES (1..32)
    # [UPSTREAM-RECALL] DESIGN.md 16.  ResNeXt trunks (e2e_*_X_101_32x8d_FPN_1x): conv2 of every bottleneck is a grouped 3x3 with NUM_GROUPS groups, a stage's
    # bottleneck width is NUM_GROUPS * WIDTH_PER_GROUP * 2^stage.  FrozenBN FPN bodies, fp32, no keypoint head.
    NUM_GROUPS: int = 1          # MODEL.RESNETS.NUM_GROUPS
    WIDTH_PER_GROUP: int = 64    # MODEL.RESNETS.WIDTH_PER_GROUP
    # [UPSTREAM-RECALL] DESIGN.md 19.  Deformable trunks (dcn/e2e_*_dconv_* and *_mdconv_*): conv2 of every bottleneck of the flagged stages (res2..res5) is a
    # deformable 3x3 -- DCNv1 (18 offsets) or, with WITH_MODULATED_DCN, DCNv2 (18 offsets + 9 mask logits).  FrozenBN FPN bodies, fp32, one offset group.
    STAGE_WITH_DCN: tuple = (False, False, False, False)   # MODEL.RESNETS.STAGE_WITH_DCN
    WITH_MODULATED_DCN: bool = False                       # MODEL.RESNETS.WITH_MODULATED_DCN

    @staticmethod
    def c4():
        """e2e_mask_rcnn_R_50_C4_1x: one stride-16 map, 15 anchors, PRE/POST_NMS_TOP_N_TEST 6000/1000 (README.md:267-269),
        ROIAlign 14x14 with sampling_ratio 0, conv5 head shared by box and mask branches, MaskRCNNC4Predictor (14x14 masks)."""
        return MaskRCNNConfig(CONV_BODY="R-50-C4", SIZE_DIVISIBILITY=16, ANCHOR_STRIDE=(16,), RPN_PRE_NMS_TOP_N_TEST=6000,
                              RPN_POST_NMS_TOP_N_TEST=1000)

    @property
    def is_c4(self):
        return self.CONV_BODY.endswith("-C4")

    @property
    def det_cap(self):
        return max(self.DETECTIONS_PER_IMG, self.DETECTIONS_CAP)


BBOX_AUG_MAX_POOL = 8192   # candidate slots per image the merge (isegmi_op_retina_postprocess) sorts in LDS


@dataclass(frozen=True)
class BBoxAugConfig:
    """[UPSTREAM-RECALL] TEST.BBOX_AUG of maskrcnn-benchmark's defaults.py: multi-scale + horizontal-flip inference of a box-only model.
    POOL_CAP is this project's: candidate slots per image over all views; a pool that overflows raises BBoxAugOverflow, nothing is truncated."""
    H_FLIP: bool = False
    SCALES: tuple = ()
    MAX_SIZE: int = 4000
    SCALE_H_FLIP: bool = False
    POOL_CAP: int = BBOX_AUG_MAX_POOL


class BBoxAugOverflow(RuntimeError):
    """The views of one image passed more candidates than BBoxAugConfig.POOL_CAP holds."""


def bbox_aug_views(image_hw, cfg, aug, min_size=None, max_size=None):
    """[UPSTREAM-RECALL] engine/bbox_aug.py: the views of one image of ORIGINAL size image_hw = (h, w), in upstream's order, as (oh, ow, hflip): the
    identity view Resize(MIN_SIZE_TEST, MAX_SIZE_TEST) (min_size / max_size override the two, as COCODemo's arguments do), its mirror image with H_FLIP,
    then for every scale s Resize(s, MAX_SIZE) and, with SCALE_H_FLIP, its mirror image."""
    from .transforms import get_size
    h, w = int(image_hw[0]), int(image_hw[1])
    first = get_size(w, h, int(min_size or cfg.MIN_SIZE_TEST), int(max_size or cfg.MAX_SIZE_TEST))
    views = [first + (False,)] + ([first + (True,)] if aug.H_FLIP else [])
    for s in aug.SCALES:
        sz = get_size(w, h, int(s), int(aug.MAX_SIZE))
        views += [sz + (False,)] + ([sz + (True,)] if aug.SCALE_H_FLIP else [])
    return views


def bbox_aug_plan(sizes_hw, cfg, aug, min_size=None, max_size=None):
    """The device-resize blob of one augmented batch: every original once, one launch per view of bbox_aug_views -- its rows name every
    image of the batch, each on its own canvas plane.  -> (transforms.ResamplePlan, [hw [n, 2] int32 per view])"""
    from .transforms import ResamplePlan
    per_image = [bbox_aug_views(hw, cfg, aug, min_size, max_size) for hw in sizes_hw]
    views = [[(i, v[k][0], v[k][1], 0, 0, 1 if v[k][2] else 0, i) for i, v in enumerate(per_image)] for k in range(len(per_image[0]))]
    return ResamplePlan(sizes_hw, views), [np.array([(e[1], e[2]) for e in view], np.int32) for view in views]


def bbox_aug_engine_side(cfg, aug, min_size=None, max_size=None):
    """The long side an engine needs for every view the plain rule's aspect allows: min(MAX_SIZE, ceil(largest short side * max / min)), not below the plain
    rule's own long side, rounded up to SIZE_DIVISIBILITY."""
    mn, mx = int(min_size or cfg.MIN_SIZE_TEST), int(max_size or cfg.MAX_SIZE_TEST)
    d = cfg.SIZE_DIVISIBILITY
    long_side = max(mx, mn)
    if aug.SCALES:
        long_side = max(long_side, min(int(aug.MAX_SIZE), -(-max(tuple(aug.SCALES) + (mn,)) * mx // mn)))
    return -(-long_side // d) * d


GROUPED_CONV_WIDTHS = (8, 16, 32, 64)   # channels per group the grouped kernel takes (csrc/conv_grouped.hip)


def resnext_check(num_groups, width_per_group):
    """THE rule of which ResNeXt trunks are built, stated once (config.py and the model classes both ask here): every stage's channels per group,
    WIDTH_PER_GROUP * 2^stage, lie in the grouped kernel's set, and the widths are multiples of 64.  Raises ValueError naming the yaml key."""
    g, w = int(num_groups), int(width_per_group)
    if g < 1:
        raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d: at least 1" % g)
    if g == 1:
        if w != 64:
            raise ValueError("MODEL.RESNETS.WIDTH_PER_GROUP=%d with NUM_GROUPS 1: the plain ResNet trunk is built at 64" % w)
        return
    for stage in range(4):
        if (w << stage) not in GROUPED_CONV_WIDTHS:
            raise ValueError("MODEL.RESNETS.WIDTH_PER_GROUP=%d gives groups of %d channels in res%d: the grouped convolution kernel takes %s per group "
                             "(WIDTH_PER_GROUP 8)" % (w, w << stage, stage + 2, ", ".join(str(v) for v in GROUPED_CONV_WIDTHS)))
    if (g * w) % 64:
        raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d x WIDTH_PER_GROUP=%d = %d: the bottleneck width must be a multiple of 64" % (g, w, g * w))


def resnext_refusals(cfg, fp16):
    """What a ResNeXt trunk (NUM_GROUPS > 1) is not built next to; ValueError naming the key."""
    resnext_check(cfg.NUM_GROUPS, cfg.WIDTH_PER_GROUP)
    if cfg.NUM_GROUPS == 1:
        return
    for bad, why in ((fp16, "fp16=True: fp16 ResNeXt is not built (the grouped convolution kernel is fp32)"),
                     (cfg.is_c4, "the C4 body (MODEL.BACKBONE.CONV_BODY %s): ResNeXt is built on the FPN bodies" % cfg.CONV_BODY),
                     (getattr(cfg, "USE_GN", False), "GroupNorm (USE_GN): ResNeXt is built on the FrozenBN bodies"),
                     (getattr(cfg, "KEYPOINT_ON", False), "MODEL.KEYPOINT_ON: Keypoint R-CNN on ResNeXt is not built")):
        if bad:
            raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d together with %s" % (cfg.NUM_GROUPS, why))


def dcn_refusals(cfg, fp16):
    """What a deformable trunk (any of STAGE_WITH_DCN) is not built next to; ValueError naming the key."""
    stages = tuple(bool(v) for v in getattr(cfg, "STAGE_WITH_DCN", ()))
    if not any(stages):
        return
    if len(stages) != 4:
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r: four flags, one per stage res2..res5" % (stages,))
    for bad, why in ((fp16, "fp16=True: the deformable convolution kernels are fp32 only"),
                     (cfg.is_c4, "the C4 body (MODEL.BACKBONE.CONV_BODY %s): deformable convolutions are built on the FPN bodies" % cfg.CONV_BODY),
                     (getattr(cfg, "USE_GN", False), "GroupNorm (USE_GN): deformable convolutions are built on the FrozenBN bodies"),
                     (getattr(cfg, "NUM_GROUPS", 1) > 1, "MODEL.RESNETS.NUM_GROUPS > 1: deformable ResNeXt is not built"),
                     (getattr(cfg, "KEYPOINT_ON", False), "MODEL.KEYPOINT_ON: Keypoint R-CNN with deformable convolutions is not built")):
        if bad:
            raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r together with %s" % (stages, why))


GN_TILE_CHANNELS = 64   # csrc/groupnorm.hip GN_TILE_C


def gn_groups(channels, num_groups, dim_per_gp, layer):
    """THE rule of which GroupNorm configurations are built, stated once (config.to_maskrcnn_config and MaskRCNN._set_gn_conv both ask here; the kernel's
    own check, gn_geometry, is the backstop): the groups divide the layer's channels, and a layer of 64 channels or more has groups of 1, 2, 4 ... 64
    channels, because the kernels cut the channels into tiles of 64 and a tile holds whole groups.  -> the layer's group count; raises ValueError that
    names the yaml key, the layer and its channel count."""
    key, val = ("DIM_PER_GP", dim_per_gp) if dim_per_gp > 0 else ("NUM_GROUPS", num_groups)
    if val <= 0 or channels % val:
        raise ValueError("MODEL.GROUP_NORM.%s=%d does not divide the %d channels of %s" % (key, val, channels, layer))
    cpg = dim_per_gp if dim_per_gp > 0 else channels // num_groups
    if channels % 4 or (channels >= GN_TILE_CHANNELS and (channels % GN_TILE_CHANNELS or GN_TILE_CHANNELS % cpg)):
        raise ValueError("MODEL.GROUP_NORM.%s=%d gives groups of %d channels in %s (%d channels): the GroupNorm kernels take channel counts that are "
                         "multiples of 4 and, from 64 channels on, multiples of 64 with group widths that divide 64" % (key, val, cpg, layer, channels))
    return channels // cpg


def gn_model_layers(box_head_conv_dim=256, mask=True):
    """(name, channels) of every distinct GroupNorm width of the gn_baselines model, for the checks that run before any weight is seen.  mask=False:
    without the mask head (MODEL.MASK_ON False)."""
    out = [("backbone.body.stem", 64)]
    for li in range(1, 5):
        out += [("backbone.body.layer%d (conv1 / conv2)" % li, 64 << (li - 1)), ("backbone.body.layer%d (conv3 / downsample)" % li, 256 << (li - 1))]
    return out + [("backbone.fpn", 256), ("MODEL.ROI_BOX_HEAD.CONV_HEAD_DIM", box_head_conv_dim)] + ([("roi_heads.mask.feature_extractor", 256)] if mask else [])


# ---------------------------------------------------------------------------------------- anchors (A.3)
def _whctrs(a):
    w = a[2] - a[0] + 1
    h = a[3] - a[1] + 1
    return w, h, a[0] + 0.5 * (w - 1), a[1] + 0.5 * (h - 1)


def _mkanchors(ws, hs, xc, yc):
    ws = ws[:, None]; hs = hs[:, None]
    return np.hstack((xc - 0.5 * (ws - 1), yc - 0.5 * (hs - 1), xc + 0.5 * (ws - 1), yc + 0.5 * (hs - 1)))


def generate_anchors(stride, size, aspect_ratios):
    anchor = np.array([1, 1, stride, stride], np.float64) - 1
    w, h, xc, yc = _whctrs(anchor)
    ratios = np.asarray(aspect_ratios, np.float64)
    ws = np.round(np.sqrt(w * h / ratios)); hs = np.round(ws * ratios)
    ra = _mkanchors(ws, hs, xc, yc)
    scales = np.array([size / stride], np.float64)
    out = []
    for i in range(ra.shape[0]):
        w, h, xc, yc = _whctrs(ra[i])
        out.append(_mkanchors(w * scales, h * scales, xc, yc))
    return np.vstack(out).astype(np.float32)


def generate_anchors_multi(stride, sizes, aspect_ratios):
    """Single-feature-map form (R-50-C4: stride 16, sizes 32..512): ratio enumeration outside, ALL scales inside, i.e.
    anchor index = ratio * len(sizes) + size (maskrcnn-benchmark generate_anchors with several sizes)."""
    anchor = np.array([1, 1, stride, stride], np.float64) - 1
    w, h, xc, yc = _whctrs(anchor)
    ratios = np.asarray(aspect_ratios, np.float64)
    ws = np.round(np.sqrt(w * h / ratios)); hs = np.round(ws * ratios)
    ra = _mkanchors(ws, hs, xc, yc)
    scales = np.asarray(sizes, np.float64) / stride
    out = []
    for i in range(ra.shape[0]):
        w, h, xc, yc = _whctrs(ra[i])
        out.append(_mkanchors(w * scales, h * scales, xc, yc))
    return np.vstack(out).astype(np.float32)


def grid_anchors(grid_h, grid_w, stride, base):
    sx = np.arange(0, grid_w * stride, stride, dtype=np.float32)
    sy = np.arange(0, grid_h * stride, stride, dtype=np.float32)
    yy, xx = np.meshgrid(sy, sx, indexing="ij")
    shifts = np.stack([xx.ravel(), yy.ravel(), xx.ravel(), yy.ravel()], 1)
    return (shifts[:, None, :] + base[None, :, :]).reshape(-1, 4).astype(np.float32)


def level_shapes(H, W):
    s = ((H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1)
    s = ((s[0] + 2 - 3) // 2 + 1, (s[1] + 2 - 3) // 2 + 1)  # C2 (stride 4)
    out = [s]
    for _ in range(3):
        s = ((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1)      # 1x1 stride 2
        out.append(s)
    out.append(((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1))  # P6
    return out


def prepare_images(images_bgr_f32, divisibility=32):
    """to_image_list (M1) for already-resized BGR 0..255 float images: subtract PIXEL_MEAN, zero-pad to a
    common size divisible by 32.  Returns (batch NHWC3 fp32, image_hw [N,2] int32)."""
    hw = np.array([im.shape[:2] for im in images_bgr_f32], np.int32)
    H = int(-(-hw[:, 0].max() // divisibility) * divisibility)
    W = int(-(-hw[:, 1].max() // divisibility) * divisibility)
    out = np.zeros((len(images_bgr_f32), H, W, 3), np.float32)
    mean = np.asarray(PIXEL_MEAN, np.float32)
    for i, im in enumerate(images_bgr_f32):
        out[i, : im.shape[0], : im.shape[1]] = np.asarray(im, np.float32) - mean
    return out, hw


KEYPOINT_LOWRES_KEY = "roi_heads.keypoint.predictor.kps_score_lowres.weight"


def pack_keypoint_deconv(w, b):
    """ConvTranspose2d(Cin, K, kernel 4, stride 2, padding 1) as ONE 3x3, pad-1 convolution with 4 * K outputs followed by a pixel shuffle:
        out[2y + py][2x + px][k] = sum over dy, dx in -1..1 of in[y + dy][x + dx][:] . W[:, k, py + 1 - 2 dy, px + 1 - 2 dx]     (kernel index outside 0..3: no tap)
    w [Cin][K][4][4] as ConvTranspose2d stores it, b [K] -> (KRSC weights [(2 py + px) * K + k][dy + 1][dx + 1][cin], the bias repeated four times)."""
    w = np.asarray(w, np.float32)
    cin, K = w.shape[:2]
    assert w.shape[2:] == (4, 4), w.shape
    w3 = np.zeros((4 * K, 3, 3, cin), np.float32)
    for py in (0, 1):
        for px in (0, 1):
            o = (2 * py + px) * K
            for dy in (-1, 0, 1):
                ky = py + 1 - 2 * dy
                for dx in (-1, 0, 1):
                    kx = px + 1 - 2 * dx
                    if 0 <= ky <= 3 and 0 <= kx <= 3:
                        w3[o:o + K, dy + 1, dx + 1, :] = w[:, :, ky, kx].T
    return w3, np.tile(np.asarray(b, np.float32), 4)


class BoxList:
    """Minimal structures/bounding_box.BoxList (M13): xyxy boxes, size=(w,h), named fields."""

    def __init__(self, bbox, image_size, mode="xyxy"):
        self.bbox = np.asarray(bbox, np.float32).reshape(-1, 4)
        self.size = tuple(image_size)
        self.mode = mode
        self.extra_fields = {}

    def add_field(self, k, v):
        self.extra_fields[k] = v

    def get_field(self, k):
        return self.extra_fields[k]

    def has_field(self, k):
        return k in self.extra_fields

    def fields(self):
        return list(self.extra_fields)

    def __len__(self):
        return self.bbox.shape[0]

    def __getitem__(self, item):
        b = BoxList(self.bbox[item], self.size, self.mode)
        for k, v in self.extra_fields.items():
            b.add_field(k, v[item])
        return b

    def resize(self, size):
        rw, rh = (float(s) / float(o) for s, o in zip(size, self.size))
        r = np.array([rw, rh, rw, rh], np.float32)
        b = BoxList(self.bbox * r, size, self.mode)
        for k, v in self.extra_fields.items():
            if k == "keypoints":   # PersonKeypoints.resize: x and y by the ratios (one fp32 multiplication each), v untouched
                v = np.asarray(v, np.float32) * np.array([rw, rh, 1.0], np.float32)
            b.add_field(k, v)
        return b


def padded_canvas(image_hw, divisibility=32):
    """to_image_list: the canvas of a batch = max height / width over its images, rounded up to SIZE_DIVISIBILITY."""
    hw = np.asarray(image_hw, np.int64).reshape(-1, 2)
    return (int(-(-hw[:, 0].max() // divisibility) * divisibility), int(-(-hw[:, 1].max() // divisibility) * divisibility))


class MaskRCNN(Engine):
    """GeneralizedRCNN engine wrapper: `model = MaskRCNN(sd, H, W)`; `preds = model(batch, image_hw)`.

    (H, W) is the LARGEST padded canvas the engine serves.  Every batch runs on its own canvas (to_image_list pads a batch to the maximum
    size of its images, rounded up to SIZE_DIVISIBILITY; the RPN sees the padding, so results depend on the canvas exactly as upstream's
    do): weights are packed once, anchors are laid out on the device per canvas, and `reserve()` sizes every buffer once."""

    KIND = 2

    def __init__(self, state_dict, H, W, cfg=MaskRCNNConfig(), max_batch=2, device=0, fp16=False):
        assert H % cfg.SIZE_DIVISIBILITY == 0 and W % cfg.SIZE_DIVISIBILITY == 0
        assert not (cfg.is_c4 and fp16), "the C4 configuration is fp32 only"
        if cfg.USE_GN and fp16:
            raise ValueError("fp16=True with GroupNorm (USE_GN): the GroupNorm kernels are fp32 only")
        if cfg.USE_GN and cfg.is_c4:
            raise ValueError("USE_GN with the C4 body is not built")
        if cfg.USE_GN:   # before the engine exists: a refused configuration costs nothing and needs no device
            for layer, ch in gn_model_layers(cfg.BOX_HEAD_CONV_DIM, mask=bool(cfg.MASK_ON)):
                gn_groups(ch, cfg.GN_NUM_GROUPS, cfg.GN_DIM_PER_GP, layer)
        if not 2 <= int(cfg.NUM_CLASSES) <= 257:
            raise ValueError("MODEL.ROI_BOX_HEAD.NUM_CLASSES=%s: the box post-processing kernels hold 2..257 classes (background included)" % (cfg.NUM_CLASSES,))
        resnext_refusals(cfg, fp16)
        dcn_refusals(cfg, fp16)
        if cfg.KEYPOINT_ON:   # what the keypoint head is built next to
            for bad, why in ((fp16, "fp16=True: the keypoint head is fp32 only"), (cfg.is_c4, "the C4 body (CONV_BODY %s): the keypoint head reads P2..P5" % cfg.CONV_BODY),
                             (cfg.USE_GN, "GroupNorm (USE_GN): the keypoint head is built on the FrozenBN bodies"),
                             (cfg.MASK_ON, "MASK_ON True: a model with both heads is not built, set MODEL.MASK_ON: False")):
                if bad:
                    raise ValueError("KEYPOINT_ON (MODEL.KEYPOINT_ON) together with " + why)
        self.cfg, self.H, self.W, self.max_batch = cfg, H, W, max_batch
        self._mask_head_in(state_dict)   # before the engine exists: MASK_ON True with a mask-less dict is refused here
        self._keypoint_head_in(state_dict)
        self.mask_on = bool(cfg.MASK_ON)
        self.keypoint_on = bool(cfg.KEYPOINT_ON)   # MODEL.KEYPOINT_ON: __call__ adds keypoints / keypoint_logits, results leave through pack_keypoint_records
        self._ratios = None
        self.mask_buf = "det.mask14" if cfg.is_c4 else "det.mask28"
        self._create(device, max_batch, H, W)
        self.fp16 = bool(fp16)
        if self.fp16:  # fp16 storage + f16 MFMA convs (BASELINE configs[4]); must precede weight loading
            self.set_param("fp16", 1.0)
        for k, v in (("mask_on", self.mask_on), ("num_classes", cfg.NUM_CLASSES), ("cls_agnostic", bool(cfg.CLS_AGNOSTIC_BBOX_REG)),
                     ("keypoint_on", self.keypoint_on), ("num_keypoints", cfg.NUM_KEYPOINTS)):
            self.set_param(k, float(v))
        if cfg.is_c4:
            self.set_param("arch_c4", 1.0)
            self._load_c4(state_dict)
        elif cfg.USE_GN:
            self._load_gn(state_dict)
        else:
            self._load(state_dict)
        if self.keypoint_on:
            self._set_keypoint_head(state_dict)
        self.set_param("stride_in_1x1", float(bool(cfg.STRIDE_IN_1X1)))
        for k, v in (("resnet_depth", cfg.depth), ("rpn_pre_nms_top_n", cfg.RPN_PRE_NMS_TOP_N_TEST),
                     ("rpn_post_nms_top_n", cfg.RPN_POST_NMS_TOP_N_TEST), ("rpn_fpn_post_nms_top_n", cfg.RPN_FPN_POST_NMS_TOP_N_TEST),
                     ("rpn_nms_thresh", cfg.RPN_NMS_THRESH), ("rpn_min_size", cfg.RPN_MIN_SIZE), ("roi_score_thresh", cfg.ROI_SCORE_THRESH),
                     ("roi_nms_thresh", cfg.ROI_NMS), ("detections_per_img", cfg.DETECTIONS_PER_IMG), ("detections_cap", cfg.DETECTIONS_CAP),
                     ("nms_ge", cfg.NMS_GE), ("nms_plus_one", cfg.NMS_PLUS_ONE), ("nms_index_order", {"score": 0, "index": 1}[cfg.NMS_OUTPUT_ORDER]),
                     ("roi_aligned", cfg.ROI_ALIGNED), ("conv_split_k", cfg.CONV_SPLIT_K)):
            self.set_param(k, float(v))
        self._d_in = _ffi.DeviceBuffer((max_batch, H, W, 3))
        self._hw = None
        self._canvas = (H, W)

    def reserve(self):
        """Size every activation / workspace / output buffer for the largest canvas and batch by running one forward + paste on a zero batch
        (buffers only ever grow, so no forward re-allocates afterwards).  Returns memory()."""
        self._d_in.zero()
        self._hw = np.tile(np.array([[self.H, self.W]], np.int32), (self.max_batch, 1))
        self._canvas = (self.H, self.W)
        self.forward_device(self.max_batch)
        if self.mask_on:   # box-only: no paste stage, no det.masks / det.mask28 -- the smaller footprint is what memory() then reports
            self.paste_device(self.H, self.W)
        self.sync()
        return self.memory()

    @property
    def box_only(self):
        """MODEL.MASK_ON False (Faster R-CNN), or a mask engine toggled with set_mask_on(False): boxes, scores and labels only."""
        return not self.mask_on

    def set_mask_on(self, on):
        """Toggle the mask head of a live engine ("mask_on" is read each forward).  Turning it on needs the mask head's weights."""
        if on and not self.has_mask_head:
            raise ValueError("set_mask_on(True): the engine was built without mask weights (MODEL.MASK_ON False)")
        self.mask_on = bool(on)
        self.set_param("mask_on", float(self.mask_on))

    def _mask_head_in(self, sd):
        """Whether the loaders take the mask head from `sd`: MASK_ON True needs its weights (ValueError naming the key otherwise); with MASK_ON False
        present roi_heads.mask.* keys are ignored."""
        has = "roi_heads.mask.predictor.mask_fcn_logits.weight" in sd
        if self.cfg.MASK_ON and not has:
            raise ValueError("MODEL.MASK_ON is True but the state dict has no roi_heads.mask.* weights: a Faster R-CNN checkpoint needs MODEL.MASK_ON: False")
        self.has_mask_head = bool(self.cfg.MASK_ON) and has
        return self.has_mask_head

    def _keypoint_head_in(self, sd):
        """KEYPOINT_ON and the state dict must agree about the keypoint head: either side without the other raises ValueError naming the key."""
        has = [k for k in sd if k.startswith("roi_heads.keypoint.")]
        if self.cfg.KEYPOINT_ON and KEYPOINT_LOWRES_KEY not in sd:
            raise ValueError("MODEL.KEYPOINT_ON is True but the state dict has no %s: a Faster R-CNN checkpoint needs MODEL.KEYPOINT_ON: False" % KEYPOINT_LOWRES_KEY)
        if not self.cfg.KEYPOINT_ON and has:
            raise ValueError("the state dict has keypoint head weights (%s) but MODEL.KEYPOINT_ON is False: a Keypoint R-CNN checkpoint needs "
                             "MODEL.KEYPOINT_ON: True" % has[0])

    def _set_keypoint_head(self, sd):
        """[UPSTREAM-RECALL] KeypointRCNNFeatureExtractor conv_fcn1.. (3x3, bias, ReLU) and KeypointRCNNPredictor kps_score_lowres, the transposed convolution
        packed as one 3x3 layer (pack_keypoint_deconv)."""
        cfg = self.cfg
        fx, cin = "roi_heads.keypoint.feature_extractor.conv_fcn", 256
        for i, cout in enumerate(cfg.KEYPOINT_CONV_LAYERS, 1):
            if "%s%d.weight" % (fx, i) not in sd:
                raise ValueError("%s%d.weight is missing: MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS names %d layers" % (fx, i, len(cfg.KEYPOINT_CONV_LAYERS)))
            w = sd["%s%d.weight" % (fx, i)]
            if w.shape != (cout, cin, 3, 3):
                raise ValueError("%s%d.weight %s: MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS asks for %s" % (fx, i, w.shape, (cout, cin, 3, 3)))
            self._set_conv_krsc("%s%d" % (fx, i), to_krsc(w), None, sd["%s%d.bias" % (fx, i)])
            cin = cout
        if "%s%d.weight" % (fx, len(cfg.KEYPOINT_CONV_LAYERS) + 1) in sd:
            raise ValueError("%s%d.weight: more layers than MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS names (%d)" % (fx, len(cfg.KEYPOINT_CONV_LAYERS) + 1, len(cfg.KEYPOINT_CONV_LAYERS)))
        wd = sd[KEYPOINT_LOWRES_KEY]
        if wd.shape != (cin, cfg.NUM_KEYPOINTS, 4, 4):
            raise ValueError("%s %s: expected (%d, MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES = %d, 4, 4)" % (KEYPOINT_LOWRES_KEY, wd.shape, cin, cfg.NUM_KEYPOINTS))
        w3, b4 = pack_keypoint_deconv(wd, sd["roi_heads.keypoint.predictor.kps_score_lowres.bias"])
        self._set_conv_krsc("roi_heads.keypoint.predictor.kps_score_lowres", w3, None, b4)

    def _set_box_predictor(self, sd, cin):
        """cls_score | bbox_pred as ONE 1x1 layer: NUM_CLASSES logits, then 4 * NUM_CLASSES deltas, or 8 with CLS_AGNOSTIC_BBOX_REG."""
        cfg = self.cfg
        wc, wb = sd["roi_heads.box.predictor.cls_score.weight"], sd["roi_heads.box.predictor.bbox_pred.weight"]
        ncls = int(cfg.NUM_CLASSES)
        if wc.shape[0] != ncls:
            raise ValueError("roi_heads.box.predictor.cls_score has %d outputs, MODEL.ROI_BOX_HEAD.NUM_CLASSES is %d" % (wc.shape[0], ncls))
        nreg, form = (8, "2 * 4 (MODEL.CLS_AGNOSTIC_BBOX_REG: True)") if cfg.CLS_AGNOSTIC_BBOX_REG else (4 * ncls, "4 * NUM_CLASSES (MODEL.CLS_AGNOSTIC_BBOX_REG: False)")
        if wb.shape[0] != nreg:
            raise ValueError("roi_heads.box.predictor.bbox_pred has %d outputs: %d classes need %d = %s" % (wb.shape[0], ncls, nreg, form))
        wp = np.concatenate([wc, wb], 0)
        bp = np.concatenate([sd["roi_heads.box.predictor.cls_score.bias"], sd["roi_heads.box.predictor.bbox_pred.bias"]])
        self._set_conv_krsc("roi_heads.box.predictor.cls_bbox", wp.reshape(ncls + nreg, 1, 1, cin), None, bp)

    def _set_mask_logits(self, sd):
        ncls = int(self.cfg.NUM_CLASSES)
        w = sd["roi_heads.mask.predictor.mask_fcn_logits.weight"]
        if w.shape[0] != ncls:
            raise ValueError("roi_heads.mask.predictor.mask_fcn_logits has %d channels, MODEL.ROI_BOX_HEAD.NUM_CLASSES is %d" % (w.shape[0], ncls))
        self._set_tensor("mask_logits.w", w.reshape(ncls, 256).astype(np.float32))
        self._set_tensor("mask_logits.b", sd["roi_heads.mask.predictor.mask_fcn_logits.bias"].astype(np.float32))

    def _set_conv2(self, sd, src, dst, stage):
        """conv2 of bottleneck `src` (stage 0..3): checked against MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP -- weight [width, width / groups, 3, 3] with
        width = groups * width_per_group * 2^stage; ValueError naming the key otherwise -- and uploaded dense (groups 1) or grouped."""
        cfg = self.cfg
        groups, wpg = int(getattr(cfg, "NUM_GROUPS", 1)), int(getattr(cfg, "WIDTH_PER_GROUP", 64))
        dcn = bool(tuple(getattr(cfg, "STAGE_WITH_DCN", ()) or (False,) * 4)[stage])
        if dcn:
            return self._set_dcn_conv2(sd, src, dst, stage)
        for k in (".conv2.offset.weight", ".conv2.conv.weight"):
            if src + k in sd:
                raise ValueError("%s%s: a deformable convolution in res%d, which MODEL.RESNETS.STAGE_WITH_DCN=%r says is plain"
                                 % (src, k, stage + 2, tuple(getattr(cfg, "STAGE_WITH_DCN", (False,) * 4))))
        key = src + ".conv2.weight"
        w = np.asarray(sd[key])
        width = (groups * wpg) << stage
        if w.ndim != 4 or w.shape[1] * groups != w.shape[0]:
            raise ValueError("%s %s: MODEL.RESNETS.NUM_GROUPS=%d needs shape[1] * %d == shape[0] (a ResNeXt checkpoint needs its NUM_GROUPS / WIDTH_PER_GROUP)"
                             % (key, tuple(w.shape), groups, groups))
        if w.shape[0] != width:
            raise ValueError("%s %s: MODEL.RESNETS.NUM_GROUPS=%d x WIDTH_PER_GROUP=%d gives a bottleneck width of %d in res%d"
                             % (key, tuple(w.shape), groups, wpg, width, stage + 2))
        scale, shift = fold_frozen_batchnorm(sd, src + ".bn2", cfg.FROZEN_BN_EPS)
        if groups == 1:
            return self._set_conv_krsc(dst + ".conv2", to_krsc(w), scale, shift)
        self._set_conv_grouped(dst + ".conv2", to_krsc(w), groups, scale, shift)   # [width, 3, 3, width / groups]

    def _set_dcn_conv2(self, sd, src, dst, stage):
        """[UPSTREAM-RECALL] maskrcnn-benchmark DFConv2d as conv2 of bottleneck `src`: <src>.conv2.offset.{weight, bias} (a plain 3x3 with 18 outputs, or 27
        with WITH_MODULATED_DCN) goes in as the engine layer <dst>.conv2.conv_offset_mask with the bias as shift; <src>.conv2.conv.weight [width, width, 3, 3]
        as the 1x1 layer <dst>.conv2 over 9 * width channels in KRSC order with bn2 folded (what the YOLACT++ loader does).  ValueError naming the key."""
        cfg = self.cfg
        width = 64 << stage
        mod = bool(cfg.WITH_MODULATED_DCN)
        if src + ".conv2.weight" in sd:
            raise ValueError("%s.conv2.weight: a plain convolution in res%d, which MODEL.RESNETS.STAGE_WITH_DCN=%r says is deformable"
                             % (src, stage + 2, tuple(cfg.STAGE_WITH_DCN)))
        for k in (".conv2.offset.weight", ".conv2.offset.bias", ".conv2.conv.weight"):
            if src + k not in sd:
                raise ValueError("%s%s is missing: MODEL.RESNETS.STAGE_WITH_DCN=%r makes conv2 of res%d deformable" % (src, k, tuple(cfg.STAGE_WITH_DCN), stage + 2))
        wo, bo, w = np.asarray(sd[src + ".conv2.offset.weight"]), np.asarray(sd[src + ".conv2.offset.bias"]), np.asarray(sd[src + ".conv2.conv.weight"])
        oc = 27 if mod else 18
        if wo.shape != (oc, width, 3, 3) or bo.shape != (oc,):
            raise ValueError("%s.conv2.offset.weight %s / bias %s: MODEL.RESNETS.WITH_MODULATED_DCN=%s needs (%d, %d, 3, 3) and (%d,)"
                             % (src, tuple(wo.shape), tuple(bo.shape), mod, oc, width, oc))
        if w.shape != (width, width, 3, 3):
            raise ValueError("%s.conv2.conv.weight %s: expected (%d, %d, 3, 3) in res%d (MODEL.RESNETS.DEFORMABLE_GROUPS 1, NUM_GROUPS 1)"
                             % (src, tuple(w.shape), width, width, stage + 2))
        if src + ".conv2.conv.bias" in sd:
            raise ValueError("%s.conv2.conv.bias: the deformable conv2 of a bottleneck has no bias" % src)
        scale, shift = fold_frozen_batchnorm(sd, src + ".bn2", cfg.FROZEN_BN_EPS)
        self._set_conv_krsc(dst + ".conv2.conv_offset_mask", to_krsc(wo), None, bo)
        self._set_conv_krsc(dst + ".conv2", to_krsc(w).reshape(width, 1, 1, 9 * width), scale, shift)

    def _load(self, sd):
        cfg = self.cfg
        w = to_krsc(sd["backbone.body.stem.conv1.weight"])
        w = np.concatenate([w, np.zeros(w.shape[:3] + (1,), np.float32)], -1)
        self._set_conv_krsc("backbone.body.stem.conv1", w, *fold_frozen_batchnorm(sd, "backbone.body.stem.bn1", cfg.FROZEN_BN_EPS))
        blocks = (3, 4, 23 if cfg.depth == 101 else 6, 3)
        for li, nb in enumerate(blocks, 1):
            for b in range(nb):
                nm = "backbone.body.layer%d.%d" % (li, b)
                for i in (1, 3):
                    self._set_conv_krsc("%s.conv%d" % (nm, i), to_krsc(sd["%s.conv%d.weight" % (nm, i)]),
                                        *fold_frozen_batchnorm(sd, "%s.bn%d" % (nm, i), cfg.FROZEN_BN_EPS))
                self._set_conv2(sd, nm, nm, li - 1)
                if b == 0:
                    self._set_conv_krsc(nm + ".downsample.0", to_krsc(sd[nm + ".downsample.0.weight"]),
                                        *fold_frozen_batchnorm(sd, nm + ".downsample.1", cfg.FROZEN_BN_EPS))
        for i in range(1, 5):
            for k in ("inner", "layer"):
                nm = "backbone.fpn.fpn_%s%d" % (k, i)
                self._set_conv_krsc(nm, to_krsc(sd[nm + ".weight"]), None, sd[nm + ".bias"])
        self._set_conv_krsc("rpn.head.conv", to_krsc(sd["rpn.head.conv.weight"]), None, sd["rpn.head.conv.bias"])
        # fused 1x1: A objectness logits followed by A*4 deltas
        wcb = np.concatenate([to_krsc(sd["rpn.head.cls_logits.weight"]), to_krsc(sd["rpn.head.bbox_pred.weight"])], 0)
        bcb = np.concatenate([sd["rpn.head.cls_logits.bias"], sd["rpn.head.bbox_pred.bias"]])
        self._set_conv_krsc("rpn.head.cls_bbox", wcb, None, bcb)
        # FC6 consumes NHWC RoI features: permute its (c,h,w) input ordering to (h,w,c) -> a 7x7 'valid' conv
        w6 = sd["roi_heads.box.feature_extractor.fc6.weight"].reshape(1024, 256, 7, 7).transpose(0, 2, 3, 1)
        self._set_conv_krsc("roi_heads.box.feature_extractor.fc6", w6, None, sd["roi_heads.box.feature_extractor.fc6.bias"])
        w7 = sd["roi_heads.box.feature_extractor.fc7.weight"].reshape(1024, 1, 1, 1024)
        self._set_conv_krsc("roi_heads.box.feature_extractor.fc7", w7, None, sd["roi_heads.box.feature_extractor.fc7.bias"])
        self._set_box_predictor(sd, 1024)
        if self._mask_head_in(sd):
            for i in range(1, 5):
                nm = "roi_heads.mask.feature_extractor.mask_fcn%d" % i
                self._set_conv_krsc(nm, to_krsc(sd[nm + ".weight"]), None, sd[nm + ".bias"])
            wd = sd["roi_heads.mask.predictor.conv5_mask.weight"]  # [Cin][Cout][2][2]
            for ab in range(4):
                wab = np.ascontiguousarray(wd[:, :, ab >> 1, ab & 1].T).reshape(256, 1, 1, 256)
                self._set_conv_krsc("roi_heads.mask.predictor.conv5_mask.%d" % ab, wab, None, sd["roi_heads.mask.predictor.conv5_mask.bias"])
            self._set_mask_logits(sd)
        # AnchorGenerator: the A base anchors per level go over; the engine lays the grid out for each batch's canvas (isegmi_op_grid_anchors)
        for l, (stride, size) in enumerate(zip(cfg.ANCHOR_STRIDE, cfg.ANCHOR_SIZES)):
            self._set_tensor("anchor_base.%d" % l, generate_anchors(stride, size, cfg.ASPECT_RATIOS))
            self.set_param("anchor_stride%d" % l, float(stride))

    def _set_gn_conv(self, sd, name, conv, norm, w=None):
        """A convolution followed by GroupNorm: the conv goes over bare (scale 1, shift 0: no bias upstream), the norm's affine as the tensors
        <name>.gn.weight / .gn.bias -- their presence is what makes the engine launch GroupNorm behind the layer."""
        for k in (".running_mean", ".running_var"):
            if norm + k in sd:
                raise ValueError("%s has running statistics: a FrozenBatchNorm layer in a USE_GN model" % norm)
        if conv + ".bias" in sd:
            raise ValueError("%s.bias: a GroupNorm convolution has no bias" % conv)
        w = to_krsc(sd[conv + ".weight"]) if w is None else w
        if w.shape[0] != sd[norm + ".weight"].shape[0] or sd[norm + ".bias"].shape != sd[norm + ".weight"].shape:
            raise ValueError("%s: affine shape %s does not match %d output channels" % (norm, sd[norm + ".weight"].shape, w.shape[0]))
        cfg = self.cfg
        gn_groups(w.shape[0], cfg.GN_NUM_GROUPS, cfg.GN_DIM_PER_GP, norm)   # refuses what the kernels do not take, here and not in the first forward
        self._set_conv_krsc(name, w)
        self._set_tensor(name + ".gn.weight", np.asarray(sd[norm + ".weight"], np.float32))
        self._set_tensor(name + ".gn.bias", np.asarray(sd[norm + ".bias"], np.float32))

    def _load_gn(self, sd):
        """[UPSTREAM-RECALL] gn_baselines state dict (weights.maskrcnn_gn_state_dict lists the names)."""
        cfg = self.cfg
        if cfg.BOX_HEAD != "FPNXconv1fcFeatureExtractor":
            raise ValueError("USE_GN is built with BOX_HEAD FPNXconv1fcFeatureExtractor only")
        for k, v in (("gn_num_groups", cfg.GN_NUM_GROUPS), ("gn_dim_per_gp", cfg.GN_DIM_PER_GP), ("gn_epsilon", cfg.GN_EPSILON)):
            self.set_param(k, float(v))
        w = to_krsc(sd["backbone.body.stem.conv1.weight"])
        w = np.concatenate([w, np.zeros(w.shape[:3] + (1,), np.float32)], -1)
        self._set_gn_conv(sd, "backbone.body.stem.conv1", "backbone.body.stem.conv1", "backbone.body.stem.bn1", w)
        for li, nb in enumerate((3, 4, 23 if cfg.depth == 101 else 6, 3), 1):
            for b in range(nb):
                nm = "backbone.body.layer%d.%d" % (li, b)
                for i in (1, 2, 3):
                    self._set_gn_conv(sd, "%s.conv%d" % (nm, i), "%s.conv%d" % (nm, i), "%s.bn%d" % (nm, i))
                if b == 0:
                    self._set_gn_conv(sd, nm + ".downsample.0", nm + ".downsample.0", nm + ".downsample.1")
        for i in range(1, 5):
            for k in ("inner", "layer"):
                nm = "backbone.fpn.fpn_%s%d" % (k, i)
                self._set_gn_conv(sd, nm, nm + ".0", nm + ".1")
        self._set_conv_krsc("rpn.head.conv", to_krsc(sd["rpn.head.conv.weight"]), None, sd["rpn.head.conv.bias"])
        wcb = np.concatenate([to_krsc(sd["rpn.head.cls_logits.weight"]), to_krsc(sd["rpn.head.bbox_pred.weight"])], 0)
        bcb = np.concatenate([sd["rpn.head.cls_logits.bias"], sd["rpn.head.bbox_pred.bias"]])
        self._set_conv_krsc("rpn.head.cls_bbox", wcb, None, bcb)
        fx = "roi_heads.box.feature_extractor"
        for i in range(cfg.BOX_HEAD_STACKED_CONVS):
            self._set_gn_conv(sd, "%s.xconvs.%d" % (fx, i), "%s.xconvs.%d" % (fx, 3 * i), "%s.xconvs.%d" % (fx, 3 * i + 1))
        if "%s.xconvs.%d.weight" % (fx, 3 * cfg.BOX_HEAD_STACKED_CONVS) in sd or fx + ".fc7.weight" in sd:
            raise ValueError("%s: more layers than NUM_STACKED_CONVS=%d convolutions and fc6" % (fx, cfg.BOX_HEAD_STACKED_CONVS))
        cd, md = cfg.BOX_HEAD_CONV_DIM, cfg.BOX_HEAD_MLP_DIM
        w6 = sd[fx + ".fc6.weight"]
        if w6.shape != (md, cd * 49):
            raise ValueError("%s.fc6.weight %s: expected (MLP_HEAD_DIM, CONV_HEAD_DIM * 7 * 7) = (%d, %d)" % (fx, w6.shape, md, cd * 49))
        self._set_conv_krsc(fx + ".fc6", w6.reshape(md, cd, 7, 7).transpose(0, 2, 3, 1), None, sd[fx + ".fc6.bias"])
        self._set_box_predictor(sd, md)
        if self._mask_head_in(sd):
            for i in range(1, 5):
                nm = "roi_heads.mask.feature_extractor.mask_fcn%d" % i
                self._set_gn_conv(sd, nm, nm + ".0", nm + ".1")
            wd = sd["roi_heads.mask.predictor.conv5_mask.weight"]  # [Cin][Cout][2][2]
            for ab in range(4):
                wab = np.ascontiguousarray(wd[:, :, ab >> 1, ab & 1].T).reshape(256, 1, 1, 256)
                self._set_conv_krsc("roi_heads.mask.predictor.conv5_mask.%d" % ab, wab, None, sd["roi_heads.mask.predictor.conv5_mask.bias"])
            self._set_mask_logits(sd)
        for l, (stride, size) in enumerate(zip(cfg.ANCHOR_STRIDE, cfg.ANCHOR_SIZES)):
            self._set_tensor("anchor_base.%d" % l, generate_anchors(stride, size, cfg.ASPECT_RATIOS))
            self.set_param("anchor_stride%d" % l, float(stride))

    def _load_bottlenecks(self, sd, src_prefix, dst_prefix, nblocks, stage=None):
        """stage (0..3): conv2 is checked against MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP and may be grouped (_set_conv2); None: the plain trunks."""
        for b in range(nblocks):
            src, dst = "%s.%d" % (src_prefix, b), "%s.%d" % (dst_prefix, b)
            for i in (1, 2, 3):
                if i == 2 and stage is not None:
                    self._set_conv2(sd, src, dst, stage)
                    continue
                self._set_conv_krsc("%s.conv%d" % (dst, i), to_krsc(sd["%s.conv%d.weight" % (src, i)]),
                                    *fold_frozen_batchnorm(sd, "%s.bn%d" % (src, i), self.cfg.FROZEN_BN_EPS))
            if b == 0:
                self._set_conv_krsc(dst + ".downsample.0", to_krsc(sd[src + ".downsample.0.weight"]),
                                    *fold_frozen_batchnorm(sd, src + ".downsample.1", self.cfg.FROZEN_BN_EPS))

    def _load_c4(self, sd):
        """R-50-C4 state dict (maskrcnn-benchmark names): backbone.body.{stem,layer1..3}, rpn.head.* (1024 ch, 15 anchors),
        roi_heads.box.feature_extractor.head.layer4.* (conv5 head, shared with the mask branch), roi_heads.box.predictor
        cls_score / bbox_pred on 2048, roi_heads.mask.predictor conv5_mask (2048 -> 256) / mask_fcn_logits."""
        cfg = self.cfg
        w = to_krsc(sd["backbone.body.stem.conv1.weight"])
        w = np.concatenate([w, np.zeros(w.shape[:3] + (1,), np.float32)], -1)
        self._set_conv_krsc("backbone.body.stem.conv1", w, *fold_frozen_batchnorm(sd, "backbone.body.stem.bn1", cfg.FROZEN_BN_EPS))
        for li, nb in enumerate((3, 4, 6), 1):
            self._load_bottlenecks(sd, "backbone.body.layer%d" % li, "backbone.body.layer%d" % li, nb)
        head = "roi_heads.box.feature_extractor.head.layer4"
        self._load_bottlenecks(sd, head, head, 3)
        self._set_conv_krsc("rpn.head.conv", to_krsc(sd["rpn.head.conv.weight"]), None, sd["rpn.head.conv.bias"])
        wcb = np.concatenate([to_krsc(sd["rpn.head.cls_logits.weight"]), to_krsc(sd["rpn.head.bbox_pred.weight"])], 0)
        bcb = np.concatenate([sd["rpn.head.cls_logits.bias"], sd["rpn.head.bbox_pred.bias"]])
        self._set_conv_krsc("rpn.head.cls_bbox", wcb, None, bcb)
        self._set_box_predictor(sd, 2048)
        if self._mask_head_in(sd):
            wd = sd["roi_heads.mask.predictor.conv5_mask.weight"]  # [Cin 2048][Cout 256][2][2]
            for ab in range(4):
                wab = np.ascontiguousarray(wd[:, :, ab >> 1, ab & 1].T).reshape(256, 1, 1, wd.shape[0])
                self._set_conv_krsc("roi_heads.mask.predictor.conv5_mask.%d" % ab, wab, None, sd["roi_heads.mask.predictor.conv5_mask.bias"])
            self._set_mask_logits(sd)
        self._set_tensor("anchor_base.0", generate_anchors_multi(16, cfg.ANCHOR_SIZES, cfg.ASPECT_RATIOS))
        self.set_param("anchor_stride0", 16.0)

    # -- execution -----------------------------------------------------------------------------
    def _set_canvas(self, H, W):
        d = self.cfg.SIZE_DIVISIBILITY
        if H % d or W % d or H > self.H or W > self.W:
            raise ValueError("canvas %dx%d: must be a multiple of %d and fit inside the engine's %dx%d" % (H, W, d, self.H, self.W))
        self._canvas = (int(H), int(W))

    def upload(self, batch_nhwc3, image_hw, slot=0):
        """An already-normalised, zero-padded fp32 batch [n, H, W, 3] (prepare_images); its (H, W) is the canvas of the next forward."""
        x = np.ascontiguousarray(batch_nhwc3, np.float32)
        assert x.ndim == 4 and x.shape[3] == 3 and x.shape[0] <= self.max_batch, x.shape
        self._set_canvas(x.shape[1], x.shape[2])
        _ffi.check(_ffi.lib().isegmi_h2d(self.input_buffer(slot).ptr, x.ctypes.data_as(C.c_void_p), x.nbytes))
        self._hw = np.ascontiguousarray(image_hw, np.int32).reshape(-1, 2)
        assert self._hw.shape[0] == x.shape[0]
        return x.shape[0]

    def upload_u8(self, images_bgr_u8, slot=0, canvas=None):
        """to_image_list on the device (M1): a list of already-resized HxWx3 uint8 BGR images (what PIL's resize returns) -> mean-subtracted,
        zero-padded fp32 batch in the input buffer, bit-identical to prepare_images() on the host; a quarter of the PCIe bytes.  The batch's
        canvas is the padded maximum of its image sizes unless `canvas` = (H, W) forces a larger one."""
        assert 0 < len(images_bgr_u8) <= self.max_batch
        ims = [np.ascontiguousarray(im) for im in images_bgr_u8]
        if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in ims):
            raise TypeError("upload_u8 takes HxWx3 uint8 images: a float batch goes through upload(batch, image_hw)")
        hw = np.array([im.shape[:2] for im in ims], np.int32)
        self._set_canvas(*(canvas or padded_canvas(hw, self.cfg.SIZE_DIVISIBILITY)))
        flat = np.concatenate([im.reshape(-1) for im in ims])
        st = self._u8_staging(slot, flat.nbytes)
        _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, flat.ctypes.data_as(C.c_void_p), flat.nbytes))
        self._front_end(st, hw, slot)
        return len(ims)

    def _front_end(self, st, hw, slot):
        """build_transform's normalisation + to_image_list on the device: image i of the staging buffer -> plane i of the canvas batch."""
        H, W = self._canvas
        assert hw[:, 0].max() <= H and hw[:, 1].max() <= W, "image larger than the padded canvas"
        d_out = self.input_buffer(slot).ptr.value
        if hw.shape[0] > 1 and (hw == hw[0]).all():   # images of one size (a canvas-grouped batch, the bench batch): ONE launch for the batch
            h, w = int(hw[0, 0]), int(hw[0, 1])
            self._preprocess_u8(st.ptr.value, hw.shape[0], h, w, d_out, h, w, H, W, PIXEL_MEAN, (1.0, 1.0, 1.0), False)
            self._hw = hw
            return
        off = 0
        for i in range(hw.shape[0]):
            h, w = int(hw[i, 0]), int(hw[i, 1])
            self._preprocess_u8(st.ptr.value + off, 1, h, w, d_out + i * H * W * 3 * 4, h, w, H, W, PIXEL_MEAN, (1.0, 1.0, 1.0), False)
            off += h * w * 3
        self._hw = hw

    def upload_u8_async(self, pinned_u8, image_hw, slot=0, canvas=None):
        """upload_u8 from a uint8 _ffi.PinnedBuffer holding the images back to back (each h x w x 3), on the engine's copy stream."""
        hw = np.ascontiguousarray(image_hw, np.int32).reshape(-1, 2)
        nbytes = int((hw[:, 0].astype(np.int64) * hw[:, 1] * 3).sum())
        assert pinned_u8.nbytes >= nbytes and hw.shape[0] <= self.max_batch
        self._set_canvas(*(canvas or padded_canvas(hw, self.cfg.SIZE_DIVISIBILITY)))
        st = self._u8_staging(slot, nbytes)
        _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, st.ptr, pinned_u8.ptr, nbytes))
        self._front_end(st, hw, slot)

    # -- the resize on the device: the ORIGINAL bytes go up, one launch makes the batch's input ----------------------------
    def original_plan(self, image_hw, min_size=None, max_size=None):
        """The blob layout (transforms.ResamplePlan) of a batch of originals of sizes image_hw [(h, w)] under the resize rule (default: the config's
        MIN_SIZE_TEST / MAX_SIZE_TEST): what upload_original_u8_async takes next to pinned memory that plan.write() filled.  -> (plan, resized hw)"""
        from .transforms import maskrcnn_resize_plan
        cfg = self.cfg
        return maskrcnn_resize_plan(image_hw, int(min_size or cfg.MIN_SIZE_TEST), int(max_size or cfg.MAX_SIZE_TEST))

    def upload_original_u8(self, images_bgr_u8, slot=0, min_size=None, max_size=None, canvas=None):
        """upload_u8(maskrcnn_resize_u8(im) for im in images) with the resize on the device: the original HxWx3 uint8 BGR images go up once (with their
        tables, one copy) and ONE launch writes the mean-subtracted, zero-padded batch -- bit-identical to the host path's input buffer."""
        assert 0 < len(images_bgr_u8) <= self.max_batch
        ims = [np.ascontiguousarray(im) for im in images_bgr_u8]
        if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in ims):
            raise TypeError("upload_original_u8 takes HxWx3 uint8 images")
        plan, hw = self.original_plan([im.shape[:2] for im in ims], min_size, max_size)
        self._set_canvas(*(canvas or padded_canvas(hw, self.cfg.SIZE_DIVISIBILITY)))
        flat = np.empty(plan.nbytes, np.uint8)
        plan.write(flat, ims)
        st = self._u8_staging(slot, plan.nbytes)
        _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, flat.ctypes.data_as(C.c_void_p), plan.nbytes))
        self._resize_front_end(st, plan, hw, slot)
        return len(ims)

    def upload_original_u8_async(self, pinned_u8, plan, hw, slot=0, canvas=None):
        """upload_original_u8 from a uint8 _ffi.PinnedBuffer that plan.write() filled ((plan, hw) = original_plan(sizes)), on the engine's copy stream."""
        assert pinned_u8.nbytes >= plan.nbytes and hw.shape[0] <= self.max_batch
        self._set_canvas(*(canvas or padded_canvas(hw, self.cfg.SIZE_DIVISIBILITY)))
        st = self._u8_staging(slot, plan.nbytes)
        _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, st.ptr, pinned_u8.ptr, plan.nbytes))
        self._resize_front_end(st, plan, hw, slot)

    def _resize_front_end(self, st, plan, hw, slot):
        H, W = self._canvas
        assert hw[:, 0].max() <= H and hw[:, 1].max() <= W, "image larger than the padded canvas"
        self._resample_u8(st, plan, 0, self.input_buffer(slot).ptr.value, hw.shape[0], H, W, PIXEL_MEAN, (1.0, 1.0, 1.0), False, 0.0)
        self._hw = np.ascontiguousarray(hw, np.int32)

    def forward_device(self, n, slot=0):
        H, W = self._canvas
        _ffi.check(_ffi.lib().isegmi_maskrcnn_forward_canvas(self._h, self.input_buffer(slot).ptr, self._hw.ctypes.data_as(C.c_void_p), n, H, W))

    # -- test-time box augmentation (TEST.BBOX_AUG) ------------------------------------------------------------
    def aug_enqueue(self, images_bgr_u8, aug, slot=0, min_size=None, max_size=None, resize="host"):
        """The whole augmented pass of one batch of ORIGINAL images, enqueued: host resizes (PIL, one per distinct size rule), ONE upload of every
        scale's bytes (a scale serves both of its views: the mirror image is made by the front end), then per view the front end, the forward up to
        the box predictor and the candidate stage, and the merge into det.*.  Afterwards the engine's current image sizes are view 0's, so
        set_output_sizes / pack_box_records work as behind a plain forward.  Call aug_check() before using det.*.  -> batch size.
        resize="device" (DESIGN.md 24): no host resize at all -- each ORIGINAL goes up once, and every size rule's view and its mirror are made from those
        bytes by one isegmi_engine_resample_u8 launch per view, bit-identical to the host path's input."""
        from .transforms import get_size, maskrcnn_resize_u8
        if resize not in ("host", "device"):
            raise ValueError("resize: 'host' (PIL) or 'device' (isegmi_engine_resample_u8; DESIGN.md 24)")
        cfg = self.cfg
        n = len(images_bgr_u8)
        assert 0 < n <= self.max_batch
        if any(np.asarray(im).dtype != np.uint8 or np.asarray(im).ndim != 3 or np.asarray(im).shape[2] != 3 for im in images_bgr_u8):
            raise TypeError("detect_aug takes the original HxWx3 uint8 BGR images")
        rules = [(int(min_size or cfg.MIN_SIZE_TEST), int(max_size or cfg.MAX_SIZE_TEST), bool(aug.H_FLIP))] + \
                [(int(s), int(aug.MAX_SIZE), bool(aug.SCALE_H_FLIP)) for s in aug.SCALES]
        groups, chunks, off, kept = [], [], 0, self._canvas
        for mn, mx, flip in rules:
            if resize == "device":
                ims = []
                hw = np.array([get_size(np.asarray(im).shape[1], np.asarray(im).shape[0], mn, mx) for im in images_bgr_u8], np.int32)
            else:
                ims = [maskrcnn_resize_u8(np.ascontiguousarray(im), mn, mx) for im in images_bgr_u8]
                hw = np.array([im.shape[:2] for im in ims], np.int32)
            canvas = padded_canvas(hw, cfg.SIZE_DIVISIBILITY)
            try:                        # a view that does not fit the engine raises here, naming the sizes, before anything is enqueued;
                self._set_canvas(*canvas)
            finally:                    # the engine's own canvas and image sizes stay what the last upload made them until the pass is really enqueued
                self._canvas = kept
            offs = []
            for im in ims:
                offs.append(off)
                chunks.append(im.reshape(-1))
                off += im.size
            groups.append((hw, canvas, offs, flip))
        plan = None
        if resize == "device":   # one launch per (size rule, mirror): its table rows name every image of the batch
            plan, _ = bbox_aug_plan([np.asarray(im).shape[:2] for im in images_bgr_u8], cfg, aug, min_size, max_size)
            flat = np.empty(plan.nbytes, np.uint8)
            plan.write(flat, [np.ascontiguousarray(im) for im in images_bgr_u8])
        else:
            flat = np.concatenate(chunks)
        self.sync()   # the staging buffer may still be read by the front end of an earlier pass
        st = self._u8_staging(slot, flat.nbytes)
        _ffi.check(_ffi.lib().isegmi_h2d(st.ptr, flat.ctypes.data_as(C.c_void_p), flat.nbytes))
        lib = _ffi.lib()
        _ffi.check(lib.isegmi_maskrcnn_aug_begin(self._h, n, int(aug.POOL_CAP)))
        hw0 = groups[0][0]
        d_out = self.input_buffer(slot).ptr.value
        view = 0
        for hw, (H, W), offs, flip in groups:
            # BoxList.resize back to view 0: float(w0 / w_view), float(h0 / h_view), computed in double like _resize_ratios
            ratios = np.ascontiguousarray(np.stack([hw0[:, 1].astype(np.float64) / hw[:, 1], hw0[:, 0].astype(np.float64) / hw[:, 0]], 1).astype(np.float32))
            hwc = np.ascontiguousarray(hw, np.int32)
            for hflip in ((False, True) if flip else (False,)):
                if plan is not None:
                    self._resample_u8(st, plan, view, d_out, n, H, W, PIXEL_MEAN, (1.0, 1.0, 1.0), False, 0.0)
                    view += 1
                for i in range(n if plan is None else 0):
                    h, w = int(hw[i, 0]), int(hw[i, 1])
                    self._preprocess_u8(st.ptr.value + offs[i], 1, h, w, d_out + i * H * W * 3 * 4, h, w, H, W, PIXEL_MEAN, (1.0, 1.0, 1.0), False, hflip)
                _ffi.check(lib.isegmi_maskrcnn_aug_view(self._h, C.c_void_p(d_out), hwc.ctypes.data_as(C.c_void_p), n, H, W, 1 if hflip else 0,
                                                        ratios.ctypes.data_as(C.c_void_p)))
        _ffi.check(lib.isegmi_maskrcnn_aug_merge(self._h))
        self._hw = np.ascontiguousarray(hw0, np.int32)
        self._canvas = groups[0][1]
        self._aug_cap = int(aug.POOL_CAP)
        return n

    def aug_check(self):
        """Synchronises and raises BBoxAugOverflow if any image's views passed more candidates than POOL_CAP (det.* must then not be used)."""
        self.sync()
        n = self._hw.shape[0]
        total = self.fetch("aug.pool_total", n)
        if (total > self._aug_cap).any():
            i = int(np.argmax(total))
            raise BBoxAugOverflow("TEST.BBOX_AUG: image %d of the batch has %d candidates over its views, POOL_CAP holds %d (at most %d): raise "
                                  "MODEL.ROI_HEADS.SCORE_THRESH or use fewer views" % (i, int(total[i]), self._aug_cap, BBOX_AUG_MAX_POOL))
        return total

    def detect_aug(self, images_bgr_u8, aug, min_size=None, max_size=None, resize="host"):
        """[UPSTREAM-RECALL] im_detect_bbox_aug: ORIGINAL HxWx3 uint8 BGR images in, one BoxList per image out -- boxes, scores, labels in view-0
        coordinates (the identity view's resized image), filter_results run once over the candidates of every view."""
        n = self.aug_enqueue(images_bgr_u8, aug, 0, min_size, max_size, resize)
        self.aug_check()
        cnt = self.fetch("det.count", n)
        box, score, label = (self.fetch(k, n) for k in ("det.box", "det.score", "det.label"))
        out = []
        for i in range(n):
            c = int(cnt[i])
            bl = BoxList(box[i, :c], (int(self._hw[i, 1]), int(self._hw[i, 0])))
            bl.add_field("scores", score[i, :c]); bl.add_field("labels", label[i, :c].astype(np.int64))
            out.append(bl)
        return out

    def paste_device(self, out_h, out_w, orig_sizes_wh=None):
        """Masker paste into (out_h, out_w); orig_sizes_wh [N,2] are the sizes boxes are resized to (default: no resize)."""
        if self.box_only:
            raise RuntimeError("paste_device: the engine is box-only (MODEL.MASK_ON False): there are no masks to paste")
        ratios = self._resize_ratios(orig_sizes_wh)
        _ffi.check(_ffi.lib().isegmi_maskrcnn_paste(self._h, ratios.ctypes.data_as(C.c_void_p), out_h, out_w))

    def _resize_ratios(self, orig_sizes_wh):
        """(out_w / w, out_h / h) per image of the last upload as float32, computed like BoxList.resize."""
        n = self._hw.shape[0]
        if orig_sizes_wh is None:
            return np.ones((n, 2), np.float32)
        o = np.asarray(orig_sizes_wh, np.float64).reshape(n, 2)
        return np.ascontiguousarray(np.stack([o[:, 0] / self._hw[:, 1], o[:, 1] / self._hw[:, 0]], 1).astype(np.float32))

    def rle_device(self, image_hw=None):
        if self.box_only:
            raise RuntimeError("rle_device: the engine is box-only (MODEL.MASK_ON False): there are no masks to encode")
        return super().rle_device(image_hw)

    def set_output_sizes(self, orig_sizes_wh=None):
        """Box-only results stage: the (w, h) the boxes of the last upload are resized to by pack_box_records (default: no resize)."""
        self._ratios = self._resize_ratios(orig_sizes_wh)

    def pack_box_records(self, dev_buffer, n_block):
        """isegmi_engine_pack_box_records: the box-only record block (isegmi.dist.coco_record_layout(..., box_only=True)) of the last forward, boxes
        in the coordinates set_output_sizes named, into dev_buffer on the results stream.  -> bytes written."""
        n = self._hw.shape[0]
        r = self._ratios if self._ratios is not None and self._ratios.shape[0] == n else np.ones((n, 2), np.float32)
        nb = C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_pack_box_records(self._h, r.ctypes.data_as(C.c_void_p), dev_buffer.ptr, dev_buffer.nbytes, int(n_block), C.byref(nb)))
        return nb.value

    def pack_keypoint_records(self, dev_buffer, n_block):
        """isegmi_engine_pack_keypoint_records: the box-only block plus kpt / kscore (isegmi.dist.coco_record_layout(..., box_only=True, keypoints=NK)),
        boxes and keypoints in the coordinates set_output_sizes named.  -> bytes written."""
        n = self._hw.shape[0]
        r = self._ratios if self._ratios is not None and self._ratios.shape[0] == n else np.ones((n, 2), np.float32)
        nb = C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_pack_keypoint_records(self._h, r.ctypes.data_as(C.c_void_p), dev_buffer.ptr, dev_buffer.nbytes, int(n_block), C.byref(nb)))
        return nb.value

    def pose_handoff(self, person_threshold, keypoint_threshold, K, d_kpts, d_score, d_slot, d_count):
        """isegmi_engine_pose_handoff: the last forward's persons as Pose2Seg takes them, keypoints in the coordinates set_output_sizes
        named, into four device buffers ([n * K, 17, 3] f32, [n, K] f32, [n, K] i32, [n] i32) on the results stream.  -> the ratios used."""
        n = self._hw.shape[0] if self._hw is not None else self.max_batch   # before the first upload the engine refuses by name
        r = self._ratios if self._ratios is not None and self._ratios.shape[0] == n else np.ones((n, 2), np.float32)
        _ffi.check(_ffi.lib().isegmi_engine_pose_handoff(self._h, r.ctypes.data_as(C.c_void_p), float(person_threshold), float(keypoint_threshold), int(K),
                                                             d_kpts.ptr, d_score.ptr, d_slot.ptr, d_count.ptr))
        return r

    def results_stream(self):
        """the stream the last forward's results (and everything packed or handed off from them) complete on"""
        return self.stream()

    def __call__(self, batch_nhwc3, image_hw=None):
        """-> list of BoxList (one per image, in network-input coordinates) with scores, labels, mask [n,1,28,28]
        (14x14 for the C4 predictor; no mask field from a box-only engine; a keypoint engine adds keypoints [n,17,3] and keypoint_logits [n,17]).  With image_hw = None the first argument is a list of already-resized uint8 BGR images and goes
        through the device front end (upload_u8: mean subtraction and padding on the GPU)."""
        n = self.upload_u8(batch_nhwc3) if image_hw is None else self.upload(batch_nhwc3, image_hw)
        return self._detect(n)

    def detect_original(self, images_bgr_u8, min_size=None, max_size=None):
        """__call__ on ORIGINAL uint8 BGR images: the resize rule runs on the device (upload_original_u8).  Same results as
        self([maskrcnn_resize_u8(im, min_size, max_size) for im in images])."""
        return self._detect(self.upload_original_u8(images_bgr_u8, 0, min_size, max_size))

    def _detect(self, n):
        self.forward_device(n)
        self.sync()
        cnt = self.fetch("det.count", n)
        box, score, label = (self.fetch(k, n) for k in ("det.box", "det.score", "det.label"))
        m28 = self.fetch(self.mask_buf, n) if self.mask_on else None
        kpt, kscore = (self.fetch("det.kpt", n), self.fetch("det.kscore", n)) if self.keypoint_on else (None, None)
        out = []
        for i in range(n):
            c = int(cnt[i])
            bl = BoxList(box[i, :c], (int(self._hw[i, 1]), int(self._hw[i, 0])))
            bl.add_field("scores", score[i, :c]); bl.add_field("labels", label[i, :c].astype(np.int64))
            if m28 is not None:
                bl.add_field("mask", m28[i, :c, None])
            if kpt is not None:
                bl.add_field("keypoints", kpt[i, :c]); bl.add_field("keypoint_logits", kscore[i, :c])
            out.append(bl)
        return out
