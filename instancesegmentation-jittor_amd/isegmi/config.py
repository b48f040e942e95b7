"""`cfg` -- the yacs-shaped config node the reference's usage snippet drives (README.md:296, 313-317):

    from isegmi.config import cfg
    cfg.merge_from_file('configs/e2e_mask_rcnn_R_50_FPN_1x.yaml')
    cfg.MODEL.WEIGHT = "weight/maskrcnn_r50.npz"            # README.md:317
    coco_demo = COCODemo(cfg, min_image_size=800, confidence_threshold=0.5)

Only the inference keys of the hot path carry meaning; training/solver/dataset keys from the yaml
(README.md:263-284) are accepted and stored untouched.  yacs itself is not in the image: this is a ~60-line stand-in.
"""
import ast
import copy

import yaml

from .maskrcnn import BBOX_AUG_MAX_POOL, BBoxAugConfig, MaskRCNNConfig, gn_groups, gn_model_layers, resnext_check


def _literal(v):
    """yacs semantics: yaml hands tuples over as strings like "(4, 8, 16)"; lists become tuples."""
    if isinstance(v, list):
        return tuple(v)
    if isinstance(v, str) and v[:1] in "([" and v[-1:] in ")]":
        try:
            return tuple(ast.literal_eval(v))
        except (ValueError, SyntaxError):
            return v
    return v


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def _merge(self, other):
        for k, v in other.items():
            if isinstance(v, dict):
                node = self.setdefault(k, CfgNode())
                if not isinstance(node, CfgNode):
                    node = self[k] = CfgNode()
                node._merge(v)
            else:
                self[k] = _literal(v)

    def merge_from_file(self, path):
        with open(path) as f:
            self._merge(yaml.safe_load(f) or {})

    def merge_from_list(self, kv):
        assert len(kv) % 2 == 0
        for key, val in zip(kv[::2], kv[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node.setdefault(p, CfgNode())
            node[parts[-1]] = _literal(val)

    def clone(self):
        return copy.deepcopy(self)


def _defaults():
    c = CfgNode()
    c._merge({
        "INPUT": {"MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333, "PIXEL_MEAN": (102.9801, 115.9465, 122.7717), "TO_BGR255": True},
        "DATALOADER": {"SIZE_DIVISIBILITY": 32},
        "TEST": {"DETECTIONS_PER_IMG": 100, # [UPSTREAM-RECALL] maskrcnn-benchmark defaults.py, TEST.BBOX_AUG
                 "BBOX_AUG": {"ENABLED": False, "H_FLIP": False, "SCALES": (), "MAX_SIZE": 4000, "SCALE_H_FLIP": False}},
        # MASK_ON: upstream's default is False; this project's is True -- the e2e_faster_rcnn_* yamls under configs/ spell it out
        "MODEL": {"META_ARCHITECTURE": "GeneralizedRCNN", "WEIGHT": "", "MASK_ON": True, "RETINANET_ON": False, "RPN_ONLY": False, "KEYPOINT_ON": False,
                  "CLS_AGNOSTIC_BBOX_REG": False,
                  "BACKBONE": {"CONV_BODY": "R-50-FPN"},
                  # [UPSTREAM-RECALL] maskrcnn-benchmark defaults.py
                  "GROUP_NORM": {"DIM_PER_GP": -1, "NUM_GROUPS": 32, "EPSILON": 1e-5},
                  "RESNETS": {"TRANS_FUNC": "BottleneckWithFixedBatchNorm", "STEM_FUNC": "StemWithFixedBatchNorm", "STRIDE_IN_1X1": True,
                              "RES5_DILATION": 1, "NUM_GROUPS": 1, "WIDTH_PER_GROUP": 64, "RES2_OUT_CHANNELS": 256, "STEM_OUT_CHANNELS": 64,
                              # [UPSTREAM-RECALL] maskrcnn-benchmark defaults.py: deformable convolutions
                              "STAGE_WITH_DCN": (False, False, False, False), "WITH_MODULATED_DCN": False, "DEFORMABLE_GROUPS": 1},
                  "FPN": {"USE_GN": False, "USE_RELU": False},
                  "ROI_BOX_HEAD": {"FEATURE_EXTRACTOR": "FPN2MLPFeatureExtractor", "USE_GN": False, "NUM_STACKED_CONVS": 4, "CONV_HEAD_DIM": 256,
                                   "MLP_HEAD_DIM": 1024, "DILATION": 1, "NUM_CLASSES": 81},
                  "RPN": {"USE_FPN": True, "ANCHOR_SIZES": (32, 64, 128, 256, 512), "ANCHOR_STRIDE": (4, 8, 16, 32, 64),
                          "ASPECT_RATIOS": (0.5, 1.0, 2.0), "PRE_NMS_TOP_N_TEST": 1000, "POST_NMS_TOP_N_TEST": 1000,
                          "FPN_POST_NMS_TOP_N_TEST": 1000, "NMS_THRESH": 0.7, "MIN_SIZE": 0},
                  "ROI_HEADS": {"SCORE_THRESH": 0.05, "NMS": 0.5, "DETECTIONS_PER_IMG": 100},
                  "ROI_MASK_HEAD": {"PREDICTOR": "MaskRCNNC4Predictor", "RESOLUTION": 28, "USE_GN": False, "DILATION": 1},
                  # [UPSTREAM-RECALL] maskrcnn-benchmark defaults.py, MODEL.ROI_KEYPOINT_HEAD
                  "ROI_KEYPOINT_HEAD": {"FEATURE_EXTRACTOR": "KeypointRCNNFeatureExtractor", "PREDICTOR": "KeypointRCNNPredictor", "POOLER_RESOLUTION": 14,
                                        "POOLER_SAMPLING_RATIO": 2, "POOLER_SCALES": (0.25, 0.125, 0.0625, 0.03125), "CONV_LAYERS": (512,) * 8,
                                        "RESOLUTION": 56, "NUM_CLASSES": 17, "SHARE_BOX_FEATURE_EXTRACTOR": False},
                  # [UPSTREAM-RECALL] maskrcnn-benchmark defaults.py, MODEL.RETINANET
                  "RETINANET": {"NUM_CLASSES": 81, "ANCHOR_SIZES": (32, 64, 128, 256, 512), "ASPECT_RATIOS": (0.5, 1.0, 2.0),
                                "ANCHOR_STRIDES": (8, 16, 32, 64, 128), "STRADDLE_THRESH": 0, "OCTAVE": 2.0, "SCALES_PER_OCTAVE": 3, "USE_C5": True,
                                "NUM_CONVS": 4, "PRIOR_PROB": 0.01, "INFERENCE_TH": 0.05, "NMS_TH": 0.4, "PRE_NMS_TOP_N": 1000}},
    })
    return c


cfg = _defaults()


def _bool(v):
    return v if isinstance(v, bool) else str(v).strip().lower() in ("true", "1", "yes")


def _resnext_config(c, body, gn_key=None):
    """[UPSTREAM-RECALL] MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP / RES2_OUT_CHANNELS / STEM_OUT_CHANNELS -> (groups, width per group).  ResNeXt
    (NUM_GROUPS > 1) is built on the FrozenBN FPN bodies with WIDTH_PER_GROUP 8; everything else raises and names its key.
    gn_key: the yaml key that asks for GroupNorm, if one does."""
    rn = c.MODEL.RESNETS
    for key, built in (("RES2_OUT_CHANNELS", 256), ("STEM_OUT_CHANNELS", 64)):
        if int(rn.get(key, built)) != built:
            raise ValueError("MODEL.RESNETS.%s=%s: the trunk is built at %d" % (key, rn[key], built))
    groups, width = int(rn.get("NUM_GROUPS", 1)), int(rn.get("WIDTH_PER_GROUP", 64))
    resnext_check(groups, width)
    if groups > 1:
        if gn_key:
            raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d with GroupNorm (%s): ResNeXt is built on the FrozenBN bodies" % (groups, gn_key))
        if str(body).endswith("-C4"):
            raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d with MODEL.BACKBONE.CONV_BODY=%r: ResNeXt is built on the FPN bodies" % (groups, body))
    return groups, width


def dcn_stages(c):
    """[UPSTREAM-RECALL] MODEL.RESNETS.STAGE_WITH_DCN -> a 4-tuple of bools (res2..res5); raises, naming the key, for anything else."""
    v = c.MODEL.RESNETS.get("STAGE_WITH_DCN", (False, False, False, False))
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 4:
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r: four flags, one per stage res2..res5" % (v,))
    return tuple(_bool(x) for x in v)


def _dcn_config(c, body, use_gn, num_groups):
    """[UPSTREAM-RECALL] MODEL.RESNETS.STAGE_WITH_DCN / WITH_MODULATED_DCN / DEFORMABLE_GROUPS -> MaskRCNNConfig fields.  Built: conv2 of
    every bottleneck of the flagged stages as DCNv1 or DCNv2 on the FrozenBN R-50-FPN / R-101-FPN bodies; everything else raises and names its key."""
    rn = c.MODEL.RESNETS
    stages = dcn_stages(c)
    if int(rn.get("DEFORMABLE_GROUPS", 1)) != 1:
        raise ValueError("MODEL.RESNETS.DEFORMABLE_GROUPS=%s: deformable convolutions are built with one offset group" % rn.DEFORMABLE_GROUPS)
    if not any(stages):
        return {}   # WITH_MODULATED_DCN without a deformable stage changes nothing upstream either
    if use_gn:
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r with GroupNorm (%s): deformable convolutions are built on the FrozenBN bodies" % (stages, use_gn))
    if num_groups > 1:
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r with MODEL.RESNETS.NUM_GROUPS=%d: deformable ResNeXt is not built" % (stages, num_groups))
    if body not in ("R-50-FPN", "R-101-FPN"):
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r with MODEL.BACKBONE.CONV_BODY=%r: deformable convolutions are built on R-50-FPN and R-101-FPN" %
                         (stages, body))
    return dict(STAGE_WITH_DCN=stages, WITH_MODULATED_DCN=_bool(rn.get("WITH_MODULATED_DCN", False)))


def _norm_config(c, body, mask_on=True):
    """The norm / head keys (MODEL.GROUP_NORM, RESNETS, FPN, ROI_BOX_HEAD, ROI_MASK_HEAD) -> MaskRCNNConfig fields.  Built: FrozenBatchNorm everywhere
    with the 2-MLP box head (today's models), or [UPSTREAM-RECALL] gn_baselines -- GroupNorm in backbone, FPN, Xconv1fc box head and mask head
    together.  Everything else raises and names the key (none silently degrade).  mask_on False (MODEL.MASK_ON: Faster R-CNN): the
    ROI_MASK_HEAD keys are not consulted, "together" is backbone + FPN + box head."""
    m = c.MODEL
    rn, fpn, bh, mh, g = m.RESNETS, m.FPN, m.ROI_BOX_HEAD, m.ROI_MASK_HEAD, m.GROUP_NORM
    trans, stem = str(rn.TRANS_FUNC), str(rn.STEM_FUNC)
    if trans not in ("BottleneckWithFixedBatchNorm", "BottleneckWithGN"):
        raise ValueError("MODEL.RESNETS.TRANS_FUNC=%r: built are BottleneckWithFixedBatchNorm and BottleneckWithGN" % trans)
    if stem not in ("StemWithFixedBatchNorm", "StemWithGN"):
        raise ValueError("MODEL.RESNETS.STEM_FUNC=%r: built are StemWithFixedBatchNorm and StemWithGN" % stem)
    for key, node in (("MODEL.RESNETS.RES5_DILATION", rn.RES5_DILATION), ("MODEL.ROI_BOX_HEAD.DILATION", bh.DILATION)) + \
                     ((("MODEL.ROI_MASK_HEAD.DILATION", mh.DILATION),) if mask_on else ()):
        if int(node) != 1:
            raise ValueError("%s=%s: dilated convolutions are not built" % (key, node))
    if _bool(fpn.USE_RELU):
        raise ValueError("MODEL.FPN.USE_RELU=True is not built")
    fx = str(bh.FEATURE_EXTRACTOR)
    if fx not in ("FPN2MLPFeatureExtractor", "FPNXconv1fcFeatureExtractor"):
        raise ValueError("MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR=%r: built are FPN2MLPFeatureExtractor and FPNXconv1fcFeatureExtractor" % fx)
    flags = (("MODEL.RESNETS.TRANS_FUNC", trans == "BottleneckWithGN"), ("MODEL.RESNETS.STEM_FUNC", stem == "StemWithGN"),
             ("MODEL.FPN.USE_GN", _bool(fpn.USE_GN)), ("MODEL.ROI_BOX_HEAD.USE_GN", _bool(bh.USE_GN))) + \
            ((("MODEL.ROI_MASK_HEAD.USE_GN", _bool(mh.USE_GN)),) if mask_on else ())
    on = [k for k, v in flags if v]
    stride_in_1x1 = _bool(rn.STRIDE_IN_1X1)
    num_groups, width_per_group = _resnext_config(c, body, on[0] if on else None)
    if not on:
        if fx != "FPN2MLPFeatureExtractor":
            raise ValueError("MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR=%r is built with GroupNorm only (USE_GN: True)" % fx)
        if not stride_in_1x1 and num_groups == 1:
            raise ValueError("MODEL.RESNETS.STRIDE_IN_1X1=False is built for the GroupNorm model only")
        if int(bh.MLP_HEAD_DIM) != 1024:
            raise ValueError("MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM=%s: FPN2MLPFeatureExtractor is built at 1024" % bh.MLP_HEAD_DIM)
        if num_groups > 1:   # ResNeXt: either stride placement (the X-101-32x8d yamls say False)
            return dict(NUM_GROUPS=num_groups, WIDTH_PER_GROUP=width_per_group, STRIDE_IN_1X1=stride_in_1x1)
        return {}
    if body.endswith("-C4"):
        raise ValueError("%s: GroupNorm is built for the FPN bodies only (MODEL.BACKBONE.CONV_BODY=%r)" % (on[0], body))
    off = [k for k, v in flags if not v]
    if off:
        raise ValueError("%s asks for GroupNorm but %s does not: GroupNorm is built for backbone, FPN, box head%s together" %
                         (on[0], off[0], " and mask head" if mask_on else ""))
    if fx != "FPNXconv1fcFeatureExtractor":
        raise ValueError("MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR=%r with MODEL.ROI_BOX_HEAD.USE_GN: only FPNXconv1fcFeatureExtractor has GroupNorm" % fx)
    groups, per = int(g.NUM_GROUPS), int(g.DIM_PER_GP)
    if (groups > 0) == (per > 0):
        raise ValueError("MODEL.GROUP_NORM: exactly one of DIM_PER_GP (%d) and NUM_GROUPS (%d) must be positive" % (per, groups))
    conv_dim, mlp_dim, nconv = int(bh.CONV_HEAD_DIM), int(bh.MLP_HEAD_DIM), int(bh.NUM_STACKED_CONVS)
    if nconv < 1:
        raise ValueError("MODEL.ROI_BOX_HEAD.NUM_STACKED_CONVS=%d: at least one convolution" % nconv)
    if conv_dim % 32 or mlp_dim % 32:
        raise ValueError("MODEL.ROI_BOX_HEAD.CONV_HEAD_DIM / MLP_HEAD_DIM must be multiples of 32 (%d, %d)" % (conv_dim, mlp_dim))
    for layer, ch in gn_model_layers(box_head_conv_dim=conv_dim, mask=mask_on):   # every GroupNorm width of the model, res5's 2048 included
        gn_groups(ch, groups, per, layer)
    return dict(USE_GN=True, GN_NUM_GROUPS=groups if per <= 0 else 32, GN_DIM_PER_GP=per if per > 0 else -1, GN_EPSILON=float(g.EPSILON),
                STRIDE_IN_1X1=stride_in_1x1, BOX_HEAD=fx, BOX_HEAD_STACKED_CONVS=nconv, BOX_HEAD_CONV_DIM=conv_dim, BOX_HEAD_MLP_DIM=mlp_dim)


def to_maskrcnn_config(c):
    """Map the yaml-keyed node onto the frozen dataclass the engine consumes; rejects what the path does not build."""
    if is_keypoint_rcnn(c):
        raise ValueError("MODEL.KEYPOINT_ON=True: a Keypoint R-CNN config (DESIGN.md 14) -- to_keypointrcnn_config maps it")
    return _two_stage_config(c)


def is_bbox_aug(c):
    """True for a yaml-keyed node that asks for test-time box augmentation (TEST.BBOX_AUG.ENABLED)."""
    return _bool(c.TEST.get("BBOX_AUG", {}).get("ENABLED", False))


def to_bbox_aug_config(c):
    """[UPSTREAM-RECALL] The yaml-keyed node of a Faster R-CNN config with TEST.BBOX_AUG.ENABLED -> (MaskRCNNConfig, BBoxAugConfig); raises, naming the
    key, for everything the augmented path is not built for.  The model side goes through the two-stage mapping."""
    m, a = c.MODEL, c.TEST.get("BBOX_AUG", {})
    if not is_bbox_aug(c):
        raise ValueError("TEST.BBOX_AUG.ENABLED=False: not a test-time augmentation config (to_maskrcnn_config maps the plain two-stage models)")
    if is_retinanet(c):
        raise ValueError("TEST.BBOX_AUG.ENABLED=True together with MODEL.RETINANET_ON: test-time box augmentation is built for the two-stage box head")
    if is_keypoint_rcnn(c):
        raise ValueError("TEST.BBOX_AUG.ENABLED=True together with MODEL.KEYPOINT_ON: the augmented path returns boxes only")
    if _bool(m.MASK_ON):
        raise ValueError("TEST.BBOX_AUG.ENABLED=True together with MODEL.MASK_ON=True: the augmented path returns boxes only (as upstream's), set MODEL.MASK_ON: False")
    body = str(m.BACKBONE.CONV_BODY)
    if body.endswith("-C4"):
        raise ValueError("TEST.BBOX_AUG.ENABLED=True with MODEL.BACKBONE.CONV_BODY=%r: test-time box augmentation is built on the FPN bodies" % body)
    ncls = int(m.ROI_BOX_HEAD.NUM_CLASSES)
    if ncls > 256:
        raise ValueError("MODEL.ROI_BOX_HEAD.NUM_CLASSES=%d with TEST.BBOX_AUG.ENABLED: the merge holds 2..256 classes (background included)" % ncls)
    scales = a.get("SCALES", ())
    if isinstance(scales, (str, bytes)) or not hasattr(scales, "__iter__"):
        raise ValueError("TEST.BBOX_AUG.SCALES=%r: a tuple of positive integers" % (scales,))
    scales = tuple(scales)
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, int) or s <= 0:
            raise ValueError("TEST.BBOX_AUG.SCALES=%r: every scale is a positive integer (got %r)" % (scales, s))
    max_size = a.get("MAX_SIZE", 4000)
    # merge_from_list parses lists and tuples only, so `test_net ... TEST.BBOX_AUG.MAX_SIZE 2000` leaves the text "2000" in the node (SCALES "(400, 600)"
    # arrives as a tuple of integers already); the other integer keys take int(...) of such text too (INPUT.MIN_SIZE_TEST, MODEL.RPN.*_TOP_N_TEST)
    if isinstance(max_size, str) and max_size.strip().isdigit():
        max_size = int(max_size)
    if isinstance(max_size, bool) or not isinstance(max_size, int) or max_size <= 0:
        raise ValueError("TEST.BBOX_AUG.MAX_SIZE=%r: a positive integer" % (max_size,))
    if scales and max_size < max(scales):
        raise ValueError("TEST.BBOX_AUG.MAX_SIZE=%d is below TEST.BBOX_AUG.SCALES=%r: the long side cannot be shorter than the short side" % (max_size, scales))
    mc = _two_stage_config(c, bbox_aug=True)
    return mc, BBoxAugConfig(H_FLIP=_bool(a.get("H_FLIP", False)), SCALES=scales, MAX_SIZE=max_size, SCALE_H_FLIP=_bool(a.get("SCALE_H_FLIP", False)),
                             POOL_CAP=BBOX_AUG_MAX_POOL)


def _two_stage_config(c, bbox_aug=False):
    body = c.MODEL.BACKBONE.CONV_BODY
    r = c.MODEL.RPN
    h = c.MODEL.ROI_HEADS
    mask_on = _bool(c.MODEL.MASK_ON)
    norm = _norm_config(c, body, mask_on)
    if body not in ("R-50-FPN", "R-101-FPN", "R-50-C4"):
        raise ValueError("built bodies: R-50-FPN, R-101-FPN, R-50-C4 (got %r)" % body)
    gn_key = "MODEL.RESNETS.TRANS_FUNC=BottleneckWithGN" if norm.get("USE_GN") else None
    dcn = _dcn_config(c, body, gn_key, int(norm.get("NUM_GROUPS", 1)))
    if _bool(c.MODEL.get("RPN_ONLY", False)):
        raise ValueError("MODEL.RPN_ONLY=True is not built (DESIGN.md 13: RPN-only models are out of scope)")
    if is_bbox_aug(c) and not bbox_aug:
        raise ValueError("TEST.BBOX_AUG.ENABLED=True: a test-time box augmentation config (DESIGN.md 23) -- to_bbox_aug_config maps it")
    # [UPSTREAM-RECALL] DESIGN.md 13: the three keys that shape the RoI heads
    ncls = int(c.MODEL.ROI_BOX_HEAD.NUM_CLASSES)
    if not 2 <= ncls <= 257:
        raise ValueError("MODEL.ROI_BOX_HEAD.NUM_CLASSES=%d: the box post-processing kernels hold 2..257 classes (background included)" % ncls)
    heads = dict(MASK_ON=mask_on, NUM_CLASSES=ncls, CLS_AGNOSTIC_BBOX_REG=_bool(c.MODEL.get("CLS_AGNOSTIC_BBOX_REG", False)))
    if body == "R-50-C4":
        # the yaml the reference prints (README.md:263-273): everything it does not set comes from maskrcnn-benchmark's
        # defaults.py -- one stride-16 map, no FPN merge, SIZE_DIVISIBILITY 0 (the engine pads to 16), 14x14 masks
        if int(r.PRE_NMS_TOP_N_TEST) > 6144 or int(r.POST_NMS_TOP_N_TEST) > 1024:
            raise ValueError("MODEL.RPN.PRE/POST_NMS_TOP_N_TEST: the single-map HIP selection kernels hold 6144 / 1024 boxes")
        return MaskRCNNConfig(CONV_BODY=body, MIN_SIZE_TEST=int(c.INPUT.MIN_SIZE_TEST), MAX_SIZE_TEST=int(c.INPUT.MAX_SIZE_TEST),
                              SIZE_DIVISIBILITY=16, ANCHOR_SIZES=tuple(r.ANCHOR_SIZES), ANCHOR_STRIDE=(16,),
                              ASPECT_RATIOS=tuple(float(x) for x in r.ASPECT_RATIOS), RPN_PRE_NMS_TOP_N_TEST=int(r.PRE_NMS_TOP_N_TEST),
                              RPN_POST_NMS_TOP_N_TEST=int(r.POST_NMS_TOP_N_TEST), RPN_NMS_THRESH=float(r.NMS_THRESH),
                              RPN_MIN_SIZE=float(r.MIN_SIZE), ROI_SCORE_THRESH=float(h.SCORE_THRESH), ROI_NMS=float(h.NMS),
                              DETECTIONS_PER_IMG=int(h.DETECTIONS_PER_IMG), **heads)
    for k in ("PRE_NMS_TOP_N_TEST", "POST_NMS_TOP_N_TEST", "FPN_POST_NMS_TOP_N_TEST"):
        if int(c.MODEL.RPN[k]) > 1024:
            raise ValueError("MODEL.RPN.%s=%d: the per-level FPN selection kernels hold at most 1024 boxes" % (k, int(c.MODEL.RPN[k])))
    return MaskRCNNConfig(depth=101 if "101" in body else 50, CONV_BODY=body, MIN_SIZE_TEST=int(c.INPUT.MIN_SIZE_TEST),
                          MAX_SIZE_TEST=int(c.INPUT.MAX_SIZE_TEST),
                          SIZE_DIVISIBILITY=int(c.DATALOADER.SIZE_DIVISIBILITY), ANCHOR_SIZES=tuple(r.ANCHOR_SIZES),
                          ANCHOR_STRIDE=tuple(r.ANCHOR_STRIDE), ASPECT_RATIOS=tuple(float(x) for x in r.ASPECT_RATIOS),
                          RPN_PRE_NMS_TOP_N_TEST=int(r.PRE_NMS_TOP_N_TEST), RPN_POST_NMS_TOP_N_TEST=int(r.POST_NMS_TOP_N_TEST),
                          RPN_FPN_POST_NMS_TOP_N_TEST=int(r.FPN_POST_NMS_TOP_N_TEST), RPN_NMS_THRESH=float(r.NMS_THRESH),
                          RPN_MIN_SIZE=float(r.MIN_SIZE), ROI_SCORE_THRESH=float(h.SCORE_THRESH), ROI_NMS=float(h.NMS),
                          DETECTIONS_PER_IMG=int(h.DETECTIONS_PER_IMG), **heads, **norm, **dcn)


def is_keypoint_rcnn(c):
    """True for a yaml-keyed node that asks for the keypoint head (MODEL.KEYPOINT_ON)."""
    return _bool(c.MODEL.get("KEYPOINT_ON", False))


def to_keypointrcnn_config(c):
    """The yaml-keyed node of an e2e_keypoint_rcnn_R_*_FPN_1x.yaml -> MaskRCNNConfig with KEYPOINT_ON; raises, naming the key, for everything that is not
    built.  The box side of the model goes through the two-stage mapping, so its refusals (RPN_ONLY, TEST.BBOX_AUG.ENABLED, class
    count, norms) hold here too."""
    import dataclasses
    m = c.MODEL
    k = m.ROI_KEYPOINT_HEAD
    if not is_keypoint_rcnn(c):
        raise ValueError("MODEL.KEYPOINT_ON=False: not a Keypoint R-CNN config (to_maskrcnn_config maps the other two-stage models)")
    if _bool(m.MASK_ON):
        raise ValueError("MODEL.MASK_ON=True together with MODEL.KEYPOINT_ON: a model with both heads is not built, set MODEL.MASK_ON: False")
    body = str(m.BACKBONE.CONV_BODY)
    if body not in ("R-50-FPN", "R-101-FPN"):
        raise ValueError("MODEL.BACKBONE.CONV_BODY=%r with MODEL.KEYPOINT_ON: the keypoint head is built on R-50-FPN and R-101-FPN (it reads P2..P5)" % body)
    if any(dcn_stages(c)):
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r with MODEL.KEYPOINT_ON: Keypoint R-CNN with deformable convolutions is not built" % (dcn_stages(c),))
    mc = _two_stage_config(c)
    if mc.NUM_GROUPS > 1:
        raise ValueError("MODEL.RESNETS.NUM_GROUPS=%d with MODEL.KEYPOINT_ON: Keypoint R-CNN on ResNeXt is not built" % mc.NUM_GROUPS)
    if mc.USE_GN:
        raise ValueError("MODEL.KEYPOINT_ON with GroupNorm (MODEL.RESNETS.TRANS_FUNC / MODEL.FPN.USE_GN ...): the keypoint head is built on the FrozenBN bodies")
    if _bool(k.SHARE_BOX_FEATURE_EXTRACTOR):
        raise ValueError("MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR=True is not built: the keypoint head has its own extractor")
    for key, built in (("FEATURE_EXTRACTOR", "KeypointRCNNFeatureExtractor"), ("PREDICTOR", "KeypointRCNNPredictor")):
        if str(k[key]) != built:
            raise ValueError("MODEL.ROI_KEYPOINT_HEAD.%s=%r: built is %s" % (key, k[key], built))
    for key, built in (("POOLER_RESOLUTION", 14), ("RESOLUTION", 56), ("POOLER_SAMPLING_RATIO", 2)):
        if int(k[key]) != built:
            raise ValueError("MODEL.ROI_KEYPOINT_HEAD.%s=%s: built at %d" % (key, k[key], built))
    if tuple(float(v) for v in k.POOLER_SCALES) != (0.25, 0.125, 0.0625, 0.03125):
        raise ValueError("MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES=%r: the pooler reads P2..P5 (1/4 .. 1/32)" % (k.POOLER_SCALES,))
    layers = tuple(int(v) for v in k.CONV_LAYERS)
    if not layers or any(v <= 0 or v % 32 for v in layers):
        raise ValueError("MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS=%r: at least one layer, widths multiples of 32" % (k.CONV_LAYERS,))
    nk = int(k.NUM_CLASSES)
    if not 1 <= nk <= 32:
        raise ValueError("MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES=%d: the decode kernel holds 1..32 keypoints" % nk)
    return dataclasses.replace(mc, KEYPOINT_ON=True, KEYPOINT_CONV_LAYERS=layers, NUM_KEYPOINTS=nk)


RETINANET_BODIES = ("R-50-FPN-RETINANET", "R-101-FPN-RETINANET")


def is_retinanet(c):
    """True for a yaml-keyed node that asks for the one-stage detector (MODEL.RETINANET_ON)."""
    return _bool(c.MODEL.get("RETINANET_ON", False))


def to_retinanet_config(c):
    """The yaml-keyed node of a retinanet/retinanet_R-*-FPN_1x.yaml -> RetinaNetConfig; raises, naming the key, for everything that is not built
    (DESIGN.md 7 and 12)."""
    from .retinanet import RETINA_MAX_TOP_N, RetinaNetConfig
    m = c.MODEL
    r, rn = m.RETINANET, m.RESNETS
    if not is_retinanet(c):
        raise ValueError("MODEL.RETINANET_ON=False: not a RetinaNet config (to_maskrcnn_config maps the two-stage models)")
    if _bool(m.MASK_ON):
        raise ValueError("MODEL.MASK_ON=True together with MODEL.RETINANET_ON: RetinaMask is not built, set MODEL.MASK_ON: False")
    if is_bbox_aug(c):
        raise ValueError("TEST.BBOX_AUG.ENABLED=True together with MODEL.RETINANET_ON: test-time box augmentation is built for the two-stage box head (DESIGN.md 23)")
    body = str(m.BACKBONE.CONV_BODY)
    if body not in RETINANET_BODIES:
        raise ValueError("MODEL.BACKBONE.CONV_BODY=%r: built RetinaNet bodies are %s" % (body, ", ".join(RETINANET_BODIES)))
    if not _bool(r.USE_C5):
        raise ValueError("MODEL.RETINANET.USE_C5=False (P6 from P5) is not built: LastLevelP6P7 reads C5")
    if int(r.NUM_CONVS) < 1:
        raise ValueError("MODEL.RETINANET.NUM_CONVS=%s: at least one tower convolution" % r.NUM_CONVS)
    if int(r.NUM_CLASSES) != 81:
        raise ValueError("MODEL.RETINANET.NUM_CLASSES=%s: built for the 80 COCO classes (81)" % r.NUM_CLASSES)
    for key, on in (("MODEL.RESNETS.TRANS_FUNC", str(rn.TRANS_FUNC) != "BottleneckWithFixedBatchNorm"),
                    ("MODEL.RESNETS.STEM_FUNC", str(rn.STEM_FUNC) != "StemWithFixedBatchNorm"), ("MODEL.FPN.USE_GN", _bool(m.FPN.USE_GN))):
        if on:
            raise ValueError("%s: RetinaNet with GroupNorm is not built (FrozenBatchNorm trunk, plain FPN)" % key)
    if _bool(m.FPN.USE_RELU):
        raise ValueError("MODEL.FPN.USE_RELU=True is not built")
    num_groups, width_per_group = _resnext_config(c, body)
    if any(dcn_stages(c)):
        raise ValueError("MODEL.RESNETS.STAGE_WITH_DCN=%r with MODEL.RETINANET_ON: RetinaNet with deformable convolutions is not built" % (dcn_stages(c),))
    if int(rn.get("DEFORMABLE_GROUPS", 1)) != 1:
        raise ValueError("MODEL.RESNETS.DEFORMABLE_GROUPS=%s: deformable convolutions are not built for RetinaNet" % rn.DEFORMABLE_GROUPS)
    if not _bool(rn.STRIDE_IN_1X1) and num_groups == 1:
        raise ValueError("MODEL.RESNETS.STRIDE_IN_1X1=False is built for the GroupNorm Mask R-CNN only")
    resnext = dict(NUM_GROUPS=num_groups, WIDTH_PER_GROUP=width_per_group, STRIDE_IN_1X1=_bool(rn.STRIDE_IN_1X1)) if num_groups > 1 else {}
    if int(rn.RES5_DILATION) != 1:
        raise ValueError("MODEL.RESNETS.RES5_DILATION=%s: dilated convolutions are not built" % rn.RES5_DILATION)
    sizes, strides = tuple(r.ANCHOR_SIZES), tuple(r.ANCHOR_STRIDES)
    if len(sizes) != 5 or len(strides) != 5 or tuple(int(s) for s in strides) != (8, 16, 32, 64, 128):
        raise ValueError("MODEL.RETINANET.ANCHOR_STRIDES=%r / ANCHOR_SIZES=%r: the P3-P7 pyramid (strides 8..128, five sizes) is the one built" % (strides, sizes))
    if not 1 <= int(r.PRE_NMS_TOP_N) <= RETINA_MAX_TOP_N:
        raise ValueError("MODEL.RETINANET.PRE_NMS_TOP_N=%s: the selection kernels hold 1..%d per level" % (r.PRE_NMS_TOP_N, RETINA_MAX_TOP_N))
    if int(c.DATALOADER.SIZE_DIVISIBILITY) <= 0 or int(c.DATALOADER.SIZE_DIVISIBILITY) % 32:
        raise ValueError("DATALOADER.SIZE_DIVISIBILITY=%s: the RetinaNet pyramid needs a multiple of 32" % c.DATALOADER.SIZE_DIVISIBILITY)
    if int(c.TEST.DETECTIONS_PER_IMG) < 1:
        raise ValueError("TEST.DETECTIONS_PER_IMG=%s: at least 1" % c.TEST.DETECTIONS_PER_IMG)
    return RetinaNetConfig(depth=101 if "101" in body else 50, CONV_BODY=body, MIN_SIZE_TEST=int(c.INPUT.MIN_SIZE_TEST), MAX_SIZE_TEST=int(c.INPUT.MAX_SIZE_TEST),
                           SIZE_DIVISIBILITY=int(c.DATALOADER.SIZE_DIVISIBILITY), NUM_CLASSES=81, ANCHOR_SIZES=tuple(int(s) for s in sizes),
                           ANCHOR_STRIDES=tuple(int(s) for s in strides), ASPECT_RATIOS=tuple(float(x) for x in r.ASPECT_RATIOS), OCTAVE=float(r.OCTAVE),
                           SCALES_PER_OCTAVE=int(r.SCALES_PER_OCTAVE), NUM_CONVS=int(r.NUM_CONVS), PRE_NMS_TOP_N=int(r.PRE_NMS_TOP_N),
                           INFERENCE_TH=float(r.INFERENCE_TH), NMS_TH=float(r.NMS_TH), DETECTIONS_PER_IMG=int(c.TEST.DETECTIONS_PER_IMG), **resnext)


# ---- darknet .cfg (YOLOv3)
_NET_KEYS = (("batch", 1), ("subdivisions", 1), ("channels", 3), ("momentum", 0.9), ("decay", 0.0005), ("angle", 0), ("saturation", 1.5),
             ("exposure", 1.5), ("hue", 0.1), ("learning_rate", 0.001), ("burn_in", 1000), ("max_batches", 500200), ("policy", "steps"),
             ("steps", "400000,450000"), ("scales", ".1,.1"))


_YOLO_TOPOLOGY = {"yolov3": "YOLOv3", "spp": "YOLOv3-SPP", "tiny": "YOLOv3-tiny"}


def yolov3_sections(ycfg):
    """The section list of yolov3.cfg / yolov3-spp.cfg / yolov3-tiny.cfg (ycfg.variant) for a YoloV3Config, from the public layer lists:
    [(section, {key: str value})], [net] first.  A [yolo] section past ycfg.masks has no mask key."""
    def conv(filters, size, stride=1, bn=True):
        d = {"batch_normalize": "1"} if bn else {}
        d.update(size=str(size), stride=str(stride), pad="1", filters=str(filters), activation="leaky" if bn else "linear")
        return ("convolutional", d)

    def pool(size, stride):
        return ("maxpool", {"size": str(size), "stride": str(stride)})
    anchors = ", ".join("%d,%d" % tuple(a) for a in ycfg.anchors)

    def predictor(s):
        d = {"mask": ",".join(str(i) for i in ycfg.masks[s])} if s < len(ycfg.masks) else {}
        d.update(anchors=anchors, classes=str(ycfg.classes), num=str(len(ycfg.anchors)), jitter=".3", ignore_thresh=".7", truth_thresh="1", random="1")
        return [conv(3 * (5 + ycfg.classes), 1, bn=False), ("yolo", d)]
    out = [("net", dict([("batch", "1"), ("subdivisions", "1"), ("width", str(ycfg.width)), ("height", str(ycfg.height))] + [(k, str(v)) for k, v in _NET_KEYS[2:]]))]
    if ycfg.variant == "tiny":
        for i in range(7):
            out.append(conv(16 << i, 3))
            if i < 6:
                out.append(pool(2, 2 if i < 5 else 1))
        out += [conv(256, 1), conv(512, 3)] + predictor(0)
        out += [("route", {"layers": "-4"}), conv(128, 1), ("upsample", {"stride": "2"}), ("route", {"layers": "-1, 8"}), conv(256, 3)] + predictor(1)
        return out
    out.append(conv(32, 3))
    for li, nb in enumerate((1, 2, 8, 8, 4)):
        ch = 32 << li
        out.append(conv(ch * 2, 3, 2))
        for _ in range(nb):
            out += [conv(ch, 1), conv(ch * 2, 3), ("shortcut", {"from": "-3", "activation": "linear"})]
    for s, m in enumerate((512, 256, 128)):
        if s:
            out += [("route", {"layers": "-4"}), conv(m, 1), ("upsample", {"stride": "2"}), ("route", {"layers": "-1, %d" % (61, 36)[s - 1]})]
        for i in range(6):
            out.append(conv(2 * m if i & 1 else m, 3 if i & 1 else 1))
            if ycfg.variant == "spp" and s == 0 and i == 2:   # the SPP block: three stride-1 pools of conv2's output, routed together with it
                out += [pool(5, 1), ("route", {"layers": "-2"}), pool(9, 1), ("route", {"layers": "-4"}), pool(13, 1), ("route", {"layers": "-1,-3,-5,-6"}),
                        conv(512, 1)]
        out += predictor(s)
    return out


def yolov3_cfg_text(ycfg):
    return "\n".join("[%s]\n%s\n" % (sec, "\n".join("%s=%s" % kv for kv in d.items())) for sec, d in yolov3_sections(ycfg))


def _cfg_sections(text):
    out = []
    for n, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if line.startswith("["):
            if not line.endswith("]"):
                raise ValueError("cfg line %d: unterminated section header %r" % (n, line))
            out.append((line[1:-1].strip(), {}))
        else:
            k, eq, v = line.partition("=")
            if not eq or not out:
                raise ValueError("cfg line %d: expected key=value inside a section, got %r" % (n, line))
            out[-1][1][k.strip()] = v.strip()
    return out


_CFG_STRUCTURAL = {"convolutional": ("batch_normalize", "filters", "size", "stride", "pad", "activation"), "shortcut": ("from", "activation"),
                   "route": ("layers",), "upsample": ("stride",), "maxpool": ("size", "stride"), "yolo": ("mask", "classes", "num")}


def _cfg_first_difference(secs, want):
    """-> (index into secs[1:] of the first section that differs from `want`, its message), (len, None) when every section of the file matches."""
    topo = want[0]
    for i, (s, d) in enumerate(secs[1:]):
        if i >= len(want[1]):
            return i, "cfg section %d [%s]: past the end of the %s topology (%d layers)" % (i, s, topo, len(want[1]))
        ws, wd = want[1][i]
        got = {k: d.get(k, "0" if k == "batch_normalize" else None) for k in _CFG_STRUCTURAL[s]}
        exp = {k: wd.get(k, "0" if k == "batch_normalize" else None) for k in _CFG_STRUCTURAL.get(ws, ())}
        norm = lambda m: {k: (v.replace(" ", "") if isinstance(v, str) else v) for k, v in m.items()}
        if s != ws or norm(got) != norm(exp):
            return i, "cfg section %d [%s] %s: the %s topology has [%s] %s here" % (i, s, norm(got), topo, ws, norm(exp))
    return len(secs) - 1, None


def parse_darknet_cfg(text, **overrides):
    """A darknet yolov3.cfg, yolov3-spp.cfg or yolov3-tiny.cfg -> YoloV3Config (canvas from [net], classes / anchors / masks from the [yolo] sections, the
    variant from the layer list; `overrides` set the inference keys a .cfg does not carry).  Exactly these three topologies are accepted (DESIGN.md 17,
    21).  The file is held against the one whose section list shares the longest prefix with it (yolov3 on a tie); any other layer list -- another filter
    count or pool size, a missing route -- raises ValueError naming the first section that differs from that topology."""
    from .yolov3 import YoloV3Config
    secs = _cfg_sections(text)
    if not secs or secs[0][0] not in ("net", "network"):
        raise ValueError("cfg: the first section must be [net]")
    net = secs[0][1]
    yolos = [d for s, d in secs if s == "yolo"]
    for i, (s, _) in enumerate(secs[1:]):
        if s not in _CFG_STRUCTURAL:
            raise ValueError("cfg section %d [%s]: not part of the YOLOv3, YOLOv3-SPP or YOLOv3-tiny topology" % (i, s))
    if not yolos:
        raise ValueError("cfg: 0 [yolo] sections; the YOLOv3 topology has three")
    try:
        nums = [int(v) for v in yolos[0]["anchors"].replace(" ", "").split(",")]
        masks = tuple(tuple(int(v) for v in y["mask"].replace(" ", "").split(",")) for y in yolos)
        base = dict(height=int(net["height"]), width=int(net["width"]), classes=int(yolos[0]["classes"]), anchors=tuple(zip(nums[0::2], nums[1::2])), masks=masks)
    except KeyError as e:
        raise ValueError("cfg: missing key %s in [net] / [yolo]" % e)
    # the topology: the one the file follows furthest (the comparison needs no valid config: classes, anchors and masks are the file's own)
    best = None
    for variant in ("yolov3", "spp", "tiny"):
        probe = YoloV3Config(variant=variant, **base)
        at, msg = _cfg_first_difference(secs, (_YOLO_TOPOLOGY[variant], yolov3_sections(probe)[1:]))
        if best is None or at > best[0]:
            best = (at, msg, variant, probe)
    _, msg, variant, probe = best
    topo, nyolo = _YOLO_TOPOLOGY[variant], len(probe.strides)
    if len(yolos) != nyolo:
        raise ValueError("cfg: %d [yolo] sections; the %s topology has %s" % (len(yolos), topo, ("two", "three")[nyolo - 2]))
    if any(len(m) != 3 for m in masks):
        raise ValueError("cfg [yolo] mask=%s: three anchors per head are built (A = 3)" % (",".join(map(str, next(m for m in masks if len(m) != 3)))))
    for y in yolos[1:]:
        if y.get("anchors", "").replace(" ", "") != yolos[0]["anchors"].replace(" ", "") or y.get("classes") != yolos[0]["classes"]:
            raise ValueError("cfg [yolo]: the %s sections must share anchors and classes" % ("two", "three")[nyolo - 2])
    ycfg = YoloV3Config(variant=variant, **dict(base, **overrides))
    ycfg.validate()
    if msg:
        raise ValueError(msg)
    want = yolov3_sections(ycfg)[1:]
    if len(secs) - 1 != len(want):
        raise ValueError("cfg: %d layers; the %s topology has %d (it ends after section %d [%s])" % (len(secs) - 1, topo, len(want), len(secs) - 2, secs[-1][0]))
    return ycfg
