"""Synthetic (seeded) weights in the upstream state-dict naming, and BN folding.

BASELINE.json's configs are all "random weights" (no network for the .pth files the reference
lists at README.md:209-221, README.md:266).  Generator per SURVEY.md 8(d): conv/FC
N(0, sqrt(2/fan_in)); BN weight U(0.5,1.5), bias N(0,0.1), mean N(0,0.1), var U(0.5,1.5); the last BN
of every bottleneck is damped (x0.25) so the 16 residual adds do not blow activations up; the
predictor layers carry recorded gains/biases so a controlled number of detections pass the
score thresholds (otherwise NMS / mask stages would see nothing).
"""
import numpy as np


def _conv(rng, cout, cin, k, gain=1.0):
    std = gain * np.sqrt(2.0 / (cin * k * k))
    return (rng.standard_normal((cout, cin, k, k)) * std).astype(np.float32)


def _bn(rng, sd, prefix, c, wscale=1.0):
    sd[prefix + ".weight"] = (rng.uniform(0.5, 1.5, c) * wscale).astype(np.float32)
    sd[prefix + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    sd[prefix + ".running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    sd[prefix + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)


def _conv_bias(rng, sd, name, cout, cin, k, gain=1.0, bias_std=0.01):
    sd[name + ".weight"] = _conv(rng, cout, cin, k, gain)
    sd[name + ".bias"] = (rng.standard_normal(cout) * bias_std).astype(np.float32)


def resnet_state_dict(rng, sd, prefix, blocks=(3, 4, 6, 3), layer_fmt="layers.%d.%d", stem_conv="conv1", stem_bn="bn1", groups=1, width_per_group=64):
    """groups / width_per_group: [UPSTREAM-RECALL] ResNeXt (MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP) -- a stage's bottleneck width is
    groups * width_per_group * 2^stage and conv2 is a grouped 3x3 whose weight is [width, width / groups, 3, 3]; the defaults are the plain ResNet."""
    sd[prefix + stem_conv + ".weight"] = _conv(rng, 64, 3, 7)
    _bn(rng, sd, prefix + stem_bn, 64)
    inpl = 64
    for li, nb in enumerate(blocks):
        planes = (groups * width_per_group) << li
        out = 256 << li
        for b in range(nb):
            nm = prefix + layer_fmt % (li, b)
            sd[nm + ".conv1.weight"] = _conv(rng, planes, inpl, 1); _bn(rng, sd, nm + ".bn1", planes)
            sd[nm + ".conv2.weight"] = _conv(rng, planes, planes // groups, 3); _bn(rng, sd, nm + ".bn2", planes)
            sd[nm + ".conv3.weight"] = _conv(rng, out, planes, 1); _bn(rng, sd, nm + ".bn3", out, 0.25)
            if b == 0:
                sd[nm + ".downsample.0.weight"] = _conv(rng, out, inpl, 1)
                _bn(rng, sd, nm + ".downsample.1", out)
            inpl = out


# Recorded calibration of the Yolact predictor (see module docstring): found with the CPU oracle on
# the seeded uniform(0,255) 550x550 image so that roughly 100 detections per image survive.
YOLACT_CONF_GAIN = 0.056
YOLACT_BG_BIAS = 10.0
YOLACT_LOC_GAIN = 0.015
YOLACT_MASK_GAIN = 0.04
YOLACT_PROTO_GAIN = 0.06


def darknet53_state_dict(rng, sd, prefix="backbone."):
    """dbolya/yolact DarkNetBackbone([1, 2, 8, 8, 4]) names: _preconv.{0,1}; layers.L.0.{0,1} = the stride-2 3x3 + BN that opens
    a layer; layers.L.B.{conv1,bn1,conv2,bn2} = DarkNetBlock B (1x1 C -> C/2, 3x3 C/2 -> C, shortcut after the activation)."""
    sd[prefix + "_preconv.0.weight"] = _conv(rng, 32, 3, 3); _bn(rng, sd, prefix + "_preconv.1", 32)
    cin = 32
    for li, nb in enumerate((1, 2, 8, 8, 4)):
        ch = 32 << li
        nm = prefix + "layers.%d" % li
        sd[nm + ".0.0.weight"] = _conv(rng, ch * 2, cin, 3); _bn(rng, sd, nm + ".0.1", ch * 2)
        cin = ch * 2
        for b in range(1, nb + 1):
            sd["%s.%d.conv1.weight" % (nm, b)] = _conv(rng, ch, cin, 1); _bn(rng, sd, "%s.%d.bn1" % (nm, b), ch)
            sd["%s.%d.conv2.weight" % (nm, b)] = _conv(rng, cin, ch, 3); _bn(rng, sd, "%s.%d.bn2" % (nm, b), cin, 0.35)


def dcn_blocks(depth, dcn_layers, dcn_interval):
    """(layer, block) pairs whose 3x3 is a DCNv2 (dbolya/yolact ResNetBackbone._make_layer: the first block of a layer when
    dcn_layers >= blocks, block i > 0 when i + dcn_layers >= blocks and i % dcn_interval == 0)."""
    out = set()
    for li, nb in enumerate((3, 4, 23 if depth == 101 else 6, 3)):
        dl = dcn_layers[li]
        for b in range(nb):
            if (b == 0 and dl >= nb) or (b > 0 and b + dl >= nb and b % dcn_interval == 0):
                out.add((li, b))
    return out


YOLACT_DCN_OFFSET_STD = 0.6   # synthetic conv_offset_mask outputs: offsets of about +-1 pixel, mask logits around 0


def yolact_state_dict(seed=1234, depth=50, num_priors=3, dcn_layers=(0, 0, 0, 0), dcn_interval=1, maskiou=False, backbone="resnet"):
    """dbolya/yolact state-dict names; depth 50 = yolact_resnet50, 101 = yolact_base / yolact_im700.
    YOLACT++ (yolact_plus_*): num_priors=9, DCNv2 3x3s per dcn_layers / dcn_interval (conv2.weight/.bias and
    conv2.conv_offset_mask.weight/.bias), maskiou=True adds maskiou_net.{0,2,4,6,8,10}."""
    rng = np.random.default_rng(seed)
    sd = {}
    if backbone == "darknet53":  # yolact_darknet53_config: C3/C4/C5 have 256/512/1024 channels
        darknet53_state_dict(rng, sd, "backbone.")
        dcn_layers = (0, 0, 0, 0)
    else:
        resnet_state_dict(rng, sd, "backbone.", blocks=(3, 4, 23 if depth == 101 else 6, 3))
    for li, b in sorted(dcn_blocks(depth, dcn_layers, dcn_interval)):
        nm = "backbone.layers.%d.%d.conv2" % (li, b)
        planes = 64 << li
        sd[nm + ".bias"] = (rng.standard_normal(planes) * 0.05).astype(np.float32)
        # conv1 outputs (post BN+ReLU) are O(1): a 3x3 x planes fan-in with this std gives offsets / logits of about OFFSET_STD
        sd[nm + ".conv_offset_mask.weight"] = (rng.standard_normal((27, planes, 3, 3)) * (YOLACT_DCN_OFFSET_STD / np.sqrt(9.0 * planes))).astype(np.float32)
        sd[nm + ".conv_offset_mask.bias"] = (rng.standard_normal(27) * 0.1).astype(np.float32)
    for i, cin in enumerate((1024, 512, 256) if backbone == "darknet53" else (2048, 1024, 512)):
        _conv_bias(rng, sd, "fpn.lat_layers.%d" % i, 256, cin, 1)
    for i in range(3):
        _conv_bias(rng, sd, "fpn.pred_layers.%d" % i, 256, 256, 3)
    for i in range(2):
        _conv_bias(rng, sd, "fpn.downsample_layers.%d" % i, 256, 256, 3)
    for i in (0, 2, 4, 8):
        _conv_bias(rng, sd, "proto_net.%d" % i, 256, 256, 3)
    _conv_bias(rng, sd, "proto_net.10", 32, 256, 1, gain=YOLACT_PROTO_GAIN)
    _conv_bias(rng, sd, "prediction_layers.0.upfeature.0", 256, 256, 3)
    A = num_priors
    _conv_bias(rng, sd, "prediction_layers.0.bbox_layer", A * 4, 256, 3, gain=YOLACT_LOC_GAIN)
    _conv_bias(rng, sd, "prediction_layers.0.conf_layer", A * 81, 256, 3, gain=YOLACT_CONF_GAIN)
    _conv_bias(rng, sd, "prediction_layers.0.mask_layer", A * 32, 256, 3, gain=YOLACT_MASK_GAIN)
    b = sd["prediction_layers.0.conf_layer.bias"].reshape(A, 81)
    b[:, 0] += YOLACT_BG_BIAS
    if maskiou:  # FastMaskIoUNet: 1 -> 8 -> 16 -> 32 -> 64 -> 128 (3x3 stride 2, no padding, ReLU) -> 80 (1x1, ReLU) -> global max
        cin = 1
        for i, cout in enumerate((8, 16, 32, 64, 128)):
            _conv_bias(rng, sd, "maskiou_net.%d" % (2 * i), cout, cin, 3, bias_std=0.05)
            cin = cout
        _conv_bias(rng, sd, "maskiou_net.10", 80, 128, 1, bias_std=0.05)
        sd["maskiou_net.10.bias"] += np.float32(0.25)  # most class maps clear the final ReLU: non-degenerate IoU predictions
    return sd


def to_krsc(w_oihw):
    return np.ascontiguousarray(np.transpose(np.asarray(w_oihw, np.float32), (0, 2, 3, 1)))


def fold_batchnorm(sd, prefix, eps=1e-5):
    """nn.BatchNorm2d eval (Yolact): scale = w/sqrt(var+eps); shift = b - mean*scale."""
    w = sd[prefix + ".weight"].astype(np.float32); b = sd[prefix + ".bias"].astype(np.float32)
    m = sd[prefix + ".running_mean"].astype(np.float32); v = sd[prefix + ".running_var"].astype(np.float32)
    scale = (w / np.sqrt(v + np.float32(eps))).astype(np.float32)
    return scale, (b - m * scale).astype(np.float32)


def fold_frozen_batchnorm(sd, prefix, eps=0.0):
    """FrozenBatchNorm2d (maskrcnn-benchmark): scale = w*rsqrt(var) (no eps); shift = b - mean*scale.
    eps > 0 is the other side of the App. A.1 fork (FrozenBatchNorm2d variants that add an eps inside the rsqrt, e.g. detectron2's 1e-5):
    scale = w*rsqrt(var + eps)."""
    w = sd[prefix + ".weight"].astype(np.float32); b = sd[prefix + ".bias"].astype(np.float32)
    m = sd[prefix + ".running_mean"].astype(np.float32); v = sd[prefix + ".running_var"].astype(np.float32)
    if eps:
        v = (v + np.float32(eps)).astype(np.float32)
    scale = (w * (np.float32(1.0) / np.sqrt(v))).astype(np.float32)
    return scale, (b - m * scale).astype(np.float32)


# ---- YOLOv3 ([UPSTREAM-RECALL] the public yolov3.cfg, unverified)
YOLO_HEAD_WIDTHS = (512, 256, 128)   # M_s of head s (s = 0 at stride 32)
# Recorded calibration of the random predictors (found with the CPU reference on seeded uniform images): a few hundred of a 64 x 96 canvas's 30 240
# (anchor, class) pairs pass objectness x class > 0.05, on every level, and their boxes overlap enough for NMS to remove some.
YOLO_HEAD_BN_SCALE = (0.55, 0.55, 0.69)   # the BN weights of head s: the layers of a head would otherwise grow the trunk's already large maps
YOLO_BOX_GAIN = 0.25
YOLO_OBJ_GAIN = 0.6
YOLO_OBJ_BIAS = -1.0
YOLO_CLS_GAIN = 0.6
YOLO_CLS_BIAS = -2.9
YOLO_CLS_BIAS_SPREAD = 0.5   # per (anchor, class): a few pairs sit near the threshold at every cell, so that small canvases have candidates too


def yolov3_layers(classes=80):
    """The 75 convolutions of yolov3.cfg in file order: (conv name, BN prefix or None, Cout, Cin, kernel).  A layer with a BN prefix is conv + BN +
    LeakyReLU(0.1) and has no bias; the three predictors (head.<s>.conv6) have a bias and no BN."""
    out = [("backbone._preconv.0", "backbone._preconv.1", 32, 3, 3)]
    cin = 32
    for li, nb in enumerate((1, 2, 8, 8, 4)):
        ch = 32 << li
        nm = "backbone.layers.%d" % li
        out.append((nm + ".0.0", nm + ".0.1", ch * 2, cin, 3))
        cin = ch * 2
        for b in range(1, nb + 1):
            out.append(("%s.%d.conv1" % (nm, b), "%s.%d.bn1" % (nm, b), ch, cin, 1))
            out.append(("%s.%d.conv2" % (nm, b), "%s.%d.bn2" % (nm, b), cin, ch, 3))
    for s, m in enumerate(YOLO_HEAD_WIDTHS):
        cin = 1024 if s == 0 else m + (512 >> (s - 1))   # concat(route 256 | C4 512) = 768, concat(route 128 | C3 256) = 384
        if s:
            out.append(("head.%d.route" % s, "head.%d.route_bn" % s, m, YOLO_HEAD_WIDTHS[s - 1], 1))
        for i in range(6):
            k = 3 if i & 1 else 1
            out.append(("head.%d.conv%d" % (s, i), "head.%d.bn%d" % (s, i), 2 * m if k == 3 else m, cin, k))
            cin = 2 * m if k == 3 else m
        out.append(("head.%d.conv6" % s, None, 3 * (5 + classes), 2 * m, 1))
    assert len(out) == 75
    return out


YOLO_VARIANTS = ("yolov3", "spp", "tiny")


def yolov3_spp_layers(classes=80):
    """The 76 convolutions of yolov3-spp.cfg in file order: yolov3's, with head.0.spp (1x1 2048 -> 512 on [mp13 | mp9 | mp5 | x]) between head.0.conv2 and
    head.0.conv3."""
    out = yolov3_layers(classes)
    at = [l[0] for l in out].index("head.0.conv3")
    out.insert(at, ("head.0.spp", "head.0.spp_bn", 512, 2048, 1))
    assert len(out) == 76
    return out


def yolov3_tiny_layers(classes=80):
    """The 13 convolutions of yolov3-tiny.cfg in file order: the trunk backbone.conv0..6 (3x3), head.0.conv0 (1x1 -> 256, the branch), conv1
    (3x3 -> 512), conv2 (predictor); head.1.route (1x1 256 -> 128), head.1.conv0 (3x3 on concat(route 128 | trunk 256) -> 256), conv1 (predictor)."""
    out, cin = [], 3
    for i in range(7):
        out.append(("backbone.conv%d" % i, "backbone.bn%d" % i, 16 << i, cin, 3))
        cin = 16 << i
    out += [("head.0.conv0", "head.0.bn0", 256, 1024, 1), ("head.0.conv1", "head.0.bn1", 512, 256, 3), ("head.0.conv2", None, 3 * (5 + classes), 512, 1),
            ("head.1.route", "head.1.route_bn", 128, 256, 1), ("head.1.conv0", "head.1.bn0", 256, 384, 3), ("head.1.conv1", None, 3 * (5 + classes), 256, 1)]
    assert len(out) == 13
    return out


def yolo_layers(variant="yolov3", classes=80):
    """The convolutions of a variant's .cfg in file order, as yolov3_layers lists them."""
    if variant not in YOLO_VARIANTS:
        raise ValueError("variant=%r: yolov3, spp or tiny" % (variant,))
    return {"yolov3": yolov3_layers, "spp": yolov3_spp_layers, "tiny": yolov3_tiny_layers}[variant](classes)


# Recorded calibration of yolov3-tiny's random weights, as above (found with the CPU reference on seeded uniform images at 64 x 96, 96 x 64 and 32 x 32):
# seven conv + BN layers without a shortcut neither grow nor damp the maps much, so only the heads' BN weights are scaled.
YOLO_TINY_HEAD_BN_SCALE = (0.8, 0.8)


def yolov3_state_dict(seed=1234, classes=80, variant="yolov3"):
    """Seeded random YOLOv3 weights: the trunk is darknet53_state_dict's, the heads are head.<s>.conv0..6 / head.<s>.bn0..5 and head.<s>.route /
    head.<s>.route_bn (s = 1, 2).  The predictors carry the recorded gains / biases above.  variant "spp" adds head.0.spp / head.0.spp_bn (drawn after
    everything else, so the other layers are the yolov3 ones of the same seed); "tiny" draws yolov3_tiny_layers' names."""
    rng = np.random.default_rng(seed)
    sd = {}
    layers = yolo_layers(variant, classes)
    if variant == "tiny":
        head_scale = YOLO_TINY_HEAD_BN_SCALE
    else:
        head_scale = YOLO_HEAD_BN_SCALE
        darknet53_state_dict(rng, sd, "backbone.")
        layers = [l for l in layers if l[0] != "head.0.spp"] + [l for l in layers if l[0] == "head.0.spp"]
    for name, bn, cout, cin, k in layers:
        if name.startswith("backbone.") and variant != "tiny":
            continue
        if name.startswith("backbone."):
            sd[name + ".weight"] = _conv(rng, cout, cin, k)
            _bn(rng, sd, bn, cout)
            continue
        if bn is not None:
            sd[name + ".weight"] = _conv(rng, cout, cin, k)
            _bn(rng, sd, bn, cout, head_scale[int(name.split('.')[1])])
            continue
        w = _conv(rng, cout, cin, k).reshape(3, 5 + classes, cin, k, k)
        b = (rng.standard_normal((3, 5 + classes)) * 0.1).astype(np.float32)
        w[:, :4] *= np.float32(YOLO_BOX_GAIN); w[:, 4] *= np.float32(YOLO_OBJ_GAIN); w[:, 5:] *= np.float32(YOLO_CLS_GAIN)
        b[:, 5:] *= np.float32(YOLO_CLS_BIAS_SPREAD / 0.1)
        b[:, 4] += np.float32(YOLO_OBJ_BIAS); b[:, 5:] += np.float32(YOLO_CLS_BIAS)
        sd[name + ".weight"] = w.reshape(cout, cin, k, k)
        sd[name + ".bias"] = b.reshape(cout)
    return sd


DARKNET_WEIGHTS_HEADER = (0, 2, 0)   # major, minor, revision: minor >= 2 means a 64-bit `seen` follows


def save_darknet_weights(sd, path, classes=80, seen=0, variant="yolov3"):
    """Write a state dict as a darknet .weights file: header (three int32, then int64 `seen`), then per convolution in cfg order bias (BN: beta), and
    for a BN layer gamma, running mean, running var, then the weight [Cout][Cin][R][S]; all float32, little endian.  variant: whose layer list
    (yolo_layers) the file follows."""
    with open(path, "wb") as f:
        f.write(np.asarray(DARKNET_WEIGHTS_HEADER, "<i4").tobytes())
        f.write(np.asarray([seen], "<i8").tobytes())
        for name, bn, cout, cin, k in yolo_layers(variant, classes):
            parts = [sd[bn + ".bias"], sd[bn + ".weight"], sd[bn + ".running_mean"], sd[bn + ".running_var"]] if bn else [sd[name + ".bias"]]
            w = np.asarray(sd[name + ".weight"], np.float32)
            if w.shape != (cout, cin, k, k) or any(np.asarray(p).shape != (cout,) for p in parts):
                raise ValueError("%s: expected a weight of shape %s and %d-element vectors" % (name, (cout, cin, k, k), cout))
            for p in parts + [w]:
                f.write(np.ascontiguousarray(p, "<f4").tobytes())


def load_darknet_weights(path, cfg=None):
    """Read a darknet yolov3 / yolov3-spp / yolov3-tiny .weights file (cfg.variant; yolov3 without a cfg) into this project's state-dict names (BN
    statistics unfolded: YoloV3 folds them with cfg.bn_eps).  The file must hold exactly the convolutions of the topology (75 / 76 / 13): one that ends
    early or has floats left over raises and names the layer."""
    classes = 80 if cfg is None else cfg.classes
    layers = yolo_layers("yolov3" if cfg is None else cfg.variant, classes)
    raw = np.fromfile(path, np.uint8)
    if raw.size < 20:
        raise ValueError("%s: shorter than the 20-byte darknet header" % path)
    major, minor, _ = np.frombuffer(raw[:12].tobytes(), "<i4")
    if major * 10 + minor < 2:
        raise ValueError("%s: header version %d.%d has a 32-bit `seen`; only the 64-bit form (0.2 and later) is read" % (path, major, minor))
    body = raw[20:]
    if body.size % 4:
        raise ValueError("%s: %d bytes after the header are not a whole number of floats" % (path, body.size))
    data = np.frombuffer(body.tobytes(), "<f4")
    sd, off = {}, 0

    def take(n, what):
        nonlocal off
        if off + n > data.size:
            raise ValueError("%s: file too short: it ran out in %s (needs %d floats at offset %d, %d left)" % (path, what, n, off, data.size - off))
        a = data[off:off + n].astype(np.float32)
        off += n
        return a
    for name, bn, cout, cin, k in layers:
        if bn:
            for key in (".bias", ".weight", ".running_mean", ".running_var"):
                sd[bn + key] = take(cout, name + " (BN" + key + ")")
        else:
            sd[name + ".bias"] = take(cout, name + " (bias)")
        sd[name + ".weight"] = take(cout * cin * k * k, name + " (weight)").reshape(cout, cin, k, k)
    if off != data.size:
        raise ValueError("%s: file too long: %d floats left after the last layer %s (another topology or class count?)" % (path, data.size - off, layers[-1][0]))
    return sd


# Recorded calibration of the Mask R-CNN predictors (found with the CPU oracle on the seeded image):
# enough RPN proposals survive NMS and roughly 100 detections per image pass SCORE_THRESH 0.05.
MRCNN_RPN_CLS_GAIN = 0.0012
MRCNN_RPN_BBOX_GAIN = 0.0001
MRCNN_CLS_GAIN = 0.0008
MRCNN_BG_BIAS = 4.5
MRCNN_BBOX_GAIN = 0.0002
MRCNN_MASK_LOGIT_GAIN = 0.0005


# Recorded calibration of the GroupNorm model's predictors (gn_baselines; found with the CPU reference tests/maskrcnn_gn_ref.py on the seeded 256 x 352
# test canvas): every normalised feature is O(1) whatever the weights, so the gains differ from the FrozenBN model's.
MRCNN_GN_RPN_CLS_GAIN = 0.05
MRCNN_GN_RPN_BBOX_GAIN = 0.005
MRCNN_GN_CLS_GAIN = 1.4
MRCNN_GN_BG_BIAS = 4.0
MRCNN_GN_BBOX_GAIN = 0.01
MRCNN_GN_MASK_LOGIT_GAIN = 0.5


def _gn(rng, sd, prefix, c, wscale=1.0):
    """GroupNorm affine: weight U(0.5, 1.5), bias N(0, 0.1); no running statistics (that is what marks the layer as GroupNorm)."""
    sd[prefix + ".weight"] = (rng.uniform(0.5, 1.5, c) * wscale).astype(np.float32)
    sd[prefix + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)


def _box_predictor_widths(num_classes, cls_agnostic):
    """(cls_score rows, bbox_pred rows) of the box predictor: MODEL.ROI_BOX_HEAD.NUM_CLASSES logits; 4 deltas per class, or two sets of four with
    MODEL.CLS_AGNOSTIC_BBOX_REG."""
    if not 2 <= int(num_classes) <= 257:
        raise ValueError("num_classes (MODEL.ROI_BOX_HEAD.NUM_CLASSES) = %s: 2..257" % (num_classes,))
    return int(num_classes), 8 if cls_agnostic else 4 * int(num_classes)


def _drop_mask_head(sd):
    """Faster R-CNN (MODEL.MASK_ON False): the mask head is drawn and dropped, so every remaining tensor equals the Mask R-CNN dict's of the same seed."""
    return {k: v for k, v in sd.items() if not k.startswith("roi_heads.mask.")}


def maskrcnn_gn_state_dict(seed=1234, depth=50, stacked_convs=4, conv_head_dim=256, mlp_head_dim=1024, mask=True, num_classes=81, cls_agnostic=False):
    """mask=False: without roi_heads.mask.* (e2e_faster_rcnn_*); num_classes / cls_agnostic size the predictors.
    [UPSTREAM-RECALL] maskrcnn-benchmark gn_baselines/e2e_mask_rcnn_R_50_FPN_1x_gn state-dict names: the norms sit where the FrozenBN sat
    (stem.bn1, bn1/bn2/bn3, downsample.1) with weight and bias only; fpn_innerK / fpn_layerK / mask_fcnK are Sequential(conv, GN) -> `.0.weight`,
    `.1.{weight,bias}`; box head xconvs.{0,3,6,9} (conv) and xconvs.{1,4,7,10} (GN), fc6, no fc7.  GN convolutions have no bias."""
    rng = np.random.default_rng(seed)
    sd = {}
    tmp = {}
    resnet_state_dict(rng, tmp, "", blocks=(3, 4, 23 if depth == 101 else 6, 3))
    for k, v in tmp.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            continue
        if k.endswith("bn3.weight"):   # the FrozenBN generator damps a block's last norm (x 0.25); GroupNorm renormalises every layer: undo it (exact)
            v = v * np.float32(4.0)
        if k.startswith("conv1.") or k.startswith("bn1."):
            sd["backbone.body.stem." + k] = v
        else:
            parts = k.split(".")
            sd["backbone.body.layer%d.%s" % (int(parts[1]) + 1, ".".join(parts[2:]))] = v
    for i, cin in enumerate((256, 512, 1024, 2048), 1):
        sd["backbone.fpn.fpn_inner%d.0.weight" % i] = _conv(rng, 256, cin, 1); _gn(rng, sd, "backbone.fpn.fpn_inner%d.1" % i, 256)
        sd["backbone.fpn.fpn_layer%d.0.weight" % i] = _conv(rng, 256, 256, 3); _gn(rng, sd, "backbone.fpn.fpn_layer%d.1" % i, 256)
    _conv_bias(rng, sd, "rpn.head.conv", 256, 256, 3)
    _conv_bias(rng, sd, "rpn.head.cls_logits", 3, 256, 1, gain=MRCNN_GN_RPN_CLS_GAIN)
    _conv_bias(rng, sd, "rpn.head.bbox_pred", 12, 256, 1, gain=MRCNN_GN_RPN_BBOX_GAIN)
    cin = 256
    for i in range(stacked_convs):
        sd["roi_heads.box.feature_extractor.xconvs.%d.weight" % (3 * i)] = _conv(rng, conv_head_dim, cin, 3)
        _gn(rng, sd, "roi_heads.box.feature_extractor.xconvs.%d" % (3 * i + 1), conv_head_dim)
        cin = conv_head_dim

    def fc(name, cout, cin, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((cout, cin)) * gain * np.sqrt(2.0 / cin)).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    ncls, nreg = _box_predictor_widths(num_classes, cls_agnostic)
    fc("roi_heads.box.feature_extractor.fc6", mlp_head_dim, conv_head_dim * 7 * 7)
    fc("roi_heads.box.predictor.cls_score", ncls, mlp_head_dim, MRCNN_GN_CLS_GAIN)
    fc("roi_heads.box.predictor.bbox_pred", nreg, mlp_head_dim, MRCNN_GN_BBOX_GAIN)
    sd["roi_heads.box.predictor.cls_score.bias"][0] += MRCNN_GN_BG_BIAS
    for i in range(1, 5):
        sd["roi_heads.mask.feature_extractor.mask_fcn%d.0.weight" % i] = _conv(rng, 256, 256, 3)
        _gn(rng, sd, "roi_heads.mask.feature_extractor.mask_fcn%d.1" % i, 256)
    sd["roi_heads.mask.predictor.conv5_mask.weight"] = (rng.standard_normal((256, 256, 2, 2)) * np.sqrt(2.0 / 256)).astype(np.float32)
    sd["roi_heads.mask.predictor.conv5_mask.bias"] = (rng.standard_normal(256) * 0.01).astype(np.float32)
    _conv_bias(rng, sd, "roi_heads.mask.predictor.mask_fcn_logits", ncls, 256, 1, gain=MRCNN_GN_MASK_LOGIT_GAIN)
    return sd if mask else _drop_mask_head(sd)


def maskrcnn_state_dict(seed=1234, depth=50, gn=False, mask=True, num_classes=81, cls_agnostic=False, groups=1, width_per_group=64,
                        stage_with_dcn=(0, 0, 0, 0), modulated=False):
    """maskrcnn-benchmark e2e_mask_rcnn_R_50/101_FPN state-dict names; gn=True: the GroupNorm model (maskrcnn_gn_state_dict).
    mask=False: the e2e_faster_rcnn_* key set (no roi_heads.mask.*); num_classes / cls_agnostic size the predictors.
    groups / width_per_group: the ResNeXt trunks (e2e_*_X_101_32x8d_FPN_1x: 32, 8); the defaults are the ResNet dicts, bit for bit.
    stage_with_dcn / modulated: [UPSTREAM-RECALL] the dcn/ models (DFConv2d names): in the flagged stages res2..res5, <block>.conv2.weight becomes
    <block>.conv2.conv.weight and <block>.conv2.offset.{weight, bias} (18 outputs, 27 when modulated) is added, drawn from a SEPARATE generator so that
    every other tensor equals the plain dict's, bit for bit."""
    dcn = tuple(bool(v) for v in stage_with_dcn)
    if len(dcn) != 4:
        raise ValueError("maskrcnn_state_dict: stage_with_dcn takes four flags (res2..res5)")
    if any(dcn) and (gn or groups != 1):
        raise ValueError("maskrcnn_state_dict: deformable stages with gn=True or groups > 1 are not built")
    if gn and groups != 1:
        raise ValueError("maskrcnn_state_dict: groups > 1 (ResNeXt) with gn=True is not built")
    if gn:
        return maskrcnn_gn_state_dict(seed, depth, mask=mask, num_classes=num_classes, cls_agnostic=cls_agnostic)
    ncls, nreg = _box_predictor_widths(num_classes, cls_agnostic)
    rng = np.random.default_rng(seed)
    sd = {}
    blocks = (3, 4, 23 if depth == 101 else 6, 3)
    # ResNet body: same tensors as torchvision but under backbone.body.{stem,layerN}
    tmp = {}
    resnet_state_dict(rng, tmp, "", blocks=blocks, groups=groups, width_per_group=width_per_group)
    for k, v in tmp.items():
        if k.startswith("conv1.") or k.startswith("bn1."):
            sd["backbone.body.stem." + k] = v
        else:  # layers.L.B.xxx -> layer{L+1}.B.xxx
            parts = k.split(".")
            sd["backbone.body.layer%d.%s" % (int(parts[1]) + 1, ".".join(parts[2:]))] = v
    for i, cin in enumerate((256, 512, 1024, 2048), 1):
        _conv_bias(rng, sd, "backbone.fpn.fpn_inner%d" % i, 256, cin, 1)
        _conv_bias(rng, sd, "backbone.fpn.fpn_layer%d" % i, 256, 256, 3)
    _conv_bias(rng, sd, "rpn.head.conv", 256, 256, 3)
    _conv_bias(rng, sd, "rpn.head.cls_logits", 3, 256, 1, gain=MRCNN_RPN_CLS_GAIN)
    _conv_bias(rng, sd, "rpn.head.bbox_pred", 12, 256, 1, gain=MRCNN_RPN_BBOX_GAIN)

    def fc(name, cout, cin, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((cout, cin)) * gain * np.sqrt(2.0 / cin)).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    fc("roi_heads.box.feature_extractor.fc6", 1024, 256 * 7 * 7)
    fc("roi_heads.box.feature_extractor.fc7", 1024, 1024)
    fc("roi_heads.box.predictor.cls_score", ncls, 1024, MRCNN_CLS_GAIN)
    fc("roi_heads.box.predictor.bbox_pred", nreg, 1024, MRCNN_BBOX_GAIN)
    sd["roi_heads.box.predictor.cls_score.bias"][0] += MRCNN_BG_BIAS
    for i in range(1, 5):
        _conv_bias(rng, sd, "roi_heads.mask.feature_extractor.mask_fcn%d" % i, 256, 256, 3)
    sd["roi_heads.mask.predictor.conv5_mask.weight"] = (rng.standard_normal((256, 256, 2, 2)) * np.sqrt(2.0 / 256)).astype(np.float32)
    sd["roi_heads.mask.predictor.conv5_mask.bias"] = (rng.standard_normal(256) * 0.01).astype(np.float32)
    _conv_bias(rng, sd, "roi_heads.mask.predictor.mask_fcn_logits", ncls, 256, 1, gain=MRCNN_MASK_LOGIT_GAIN)
    if any(dcn):
        drng = np.random.default_rng([int(seed), 0xDC2])   # the deformable layers' own stream: the draws above are the plain dict's
        oc = 27 if modulated else 18
        for li, nb in enumerate(blocks, 1):
            if not dcn[li - 1]:
                continue
            planes = 64 << (li - 1)
            for b in range(nb):
                nm = "backbone.body.layer%d.%d.conv2" % (li, b)
                sd[nm + ".conv.weight"] = sd.pop(nm + ".weight")
                # conv1 outputs (post BN + ReLU) are O(1): offsets of about +-1 pixel, mask logits around 0 (as YOLACT_DCN_OFFSET_STD)
                sd[nm + ".offset.weight"] = (drng.standard_normal((oc, planes, 3, 3)) * (YOLACT_DCN_OFFSET_STD / np.sqrt(9.0 * planes))).astype(np.float32)
                sd[nm + ".offset.bias"] = (drng.standard_normal(oc) * 0.1).astype(np.float32)
    return sd if mask else _drop_mask_head(sd)


# Recorded calibration of the RetinaNet predictors (found with the CPU reference tests/retinanet_ref.py on the seeded 256 x 352 test canvas of
# tests/maskrcnn_gn_common.small_images): the tail must see all of its cases at once -- a (level, image) with more than PRE_NMS_TOP_N candidates, one
# with a few, more than DETECTIONS_PER_IMG detections before the cut, several classes.  The class bias plays the part of upstream's prior-probability
# initialisation (-log((1 - pi) / pi)); a per-class spread keeps some classes above the others.
RETINA_CLS_GAIN = 0.0003
RETINA_CLS_BIAS = -4.5
RETINA_CLS_BIAS_SPREAD = 0.5
RETINA_BBOX_GAIN = 0.0004


def retinanet_state_dict(seed=1234, depth=50, num_convs=4, cls_bias=None, groups=1, width_per_group=64):
    """[UPSTREAM-RECALL] maskrcnn-benchmark retinanet_R-50/101-FPN state-dict names: backbone.body.* (the FrozenBN trunk), backbone.fpn.fpn_inner{2,3,4} /
    fpn_layer{2,3,4} (C2 has neither), backbone.fpn.top_blocks.{p6,p7}, rpn.head.cls_tower.{0,2,4,6} / bbox_tower.{0,2,4,6} (the odd indices are the
    ReLUs), rpn.head.cls_logits (9 x 80) and rpn.head.bbox_pred (9 x 4).  cls_bias: the constant part of the cls_logits bias (default RETINA_CLS_BIAS)."""
    rng = np.random.default_rng(seed)
    sd = {}
    tmp = {}
    resnet_state_dict(rng, tmp, "", blocks=(3, 4, 23 if depth == 101 else 6, 3), groups=groups, width_per_group=width_per_group)   # (groups > 1: retinanet_X_101_32x8d_FPN_1x)
    for k, v in tmp.items():
        if k.startswith("conv1.") or k.startswith("bn1."):
            sd["backbone.body.stem." + k] = v
        else:
            parts = k.split(".")
            sd["backbone.body.layer%d.%s" % (int(parts[1]) + 1, ".".join(parts[2:]))] = v
    for i, cin in ((2, 512), (3, 1024), (4, 2048)):
        _conv_bias(rng, sd, "backbone.fpn.fpn_inner%d" % i, 256, cin, 1)
        _conv_bias(rng, sd, "backbone.fpn.fpn_layer%d" % i, 256, 256, 3)
    _conv_bias(rng, sd, "backbone.fpn.top_blocks.p6", 256, 2048, 3)
    _conv_bias(rng, sd, "backbone.fpn.top_blocks.p7", 256, 256, 3)
    for i in range(num_convs):
        _conv_bias(rng, sd, "rpn.head.cls_tower.%d" % (2 * i), 256, 256, 3)
        _conv_bias(rng, sd, "rpn.head.bbox_tower.%d" % (2 * i), 256, 256, 3)
    _conv_bias(rng, sd, "rpn.head.cls_logits", 9 * 80, 256, 3, gain=RETINA_CLS_GAIN)
    _conv_bias(rng, sd, "rpn.head.bbox_pred", 9 * 4, 256, 3, gain=RETINA_BBOX_GAIN)
    b = sd["rpn.head.cls_logits.bias"].reshape(9, 80)
    b += np.float32(RETINA_CLS_BIAS if cls_bias is None else cls_bias)
    b += (rng.standard_normal(80) * RETINA_CLS_BIAS_SPREAD).astype(np.float32)[None, :]
    return sd


# Recorded calibration of the R-50-C4 heads on the seeded uniform(0,255) image (same intent as above: about a thousand
# proposals out of the 6000 pre-NMS candidates and about a hundred detections above 0.05).
C4_RPN_CLS_GAIN = 0.0012
C4_RPN_BBOX_GAIN = 0.0001
C4_CLS_GAIN = 0.0011
C4_BG_BIAS = 3.6
C4_BBOX_GAIN = 0.0002
C4_MASK_LOGIT_GAIN = 0.0005


def maskrcnn_c4_state_dict(seed=1234, mask=True, num_classes=81, cls_agnostic=False):
    """maskrcnn-benchmark e2e_mask_rcnn_R_50_C4_1x state-dict names: backbone.body.{stem,layer1..3}; rpn.head on 1024 channels with
    15 anchors; roi_heads.box.feature_extractor.head.layer4 (conv5 head, shared with the mask branch); FastRCNNPredictor on 2048;
    MaskRCNNC4Predictor (ConvTranspose 2048 -> 256, 1x1 -> 81).  mask=False: e2e_faster_rcnn_R_50_C4_1x (no roi_heads.mask.*, the shared
    extractor's mask-side alias included); num_classes / cls_agnostic size the predictors."""
    ncls, nreg = _box_predictor_widths(num_classes, cls_agnostic)
    rng = np.random.default_rng(seed)
    sd = {}
    tmp = {}
    resnet_state_dict(rng, tmp, "", blocks=(3, 4, 6, 3))
    for k, v in tmp.items():
        if k.startswith("conv1.") or k.startswith("bn1."):
            sd["backbone.body.stem." + k] = v
            continue
        parts = k.split(".")
        li = int(parts[1]) + 1
        rest = ".".join(parts[2:])
        if li <= 3:
            sd["backbone.body.layer%d.%s" % (li, rest)] = v
        else:
            sd["roi_heads.box.feature_extractor.head.layer4." + rest] = v
            sd["roi_heads.mask.feature_extractor.head.layer4." + rest] = v  # SHARE_BOX_FEATURE_EXTRACTOR: the same module
    _conv_bias(rng, sd, "rpn.head.conv", 1024, 1024, 3)
    _conv_bias(rng, sd, "rpn.head.cls_logits", 15, 1024, 1, gain=C4_RPN_CLS_GAIN)
    _conv_bias(rng, sd, "rpn.head.bbox_pred", 60, 1024, 1, gain=C4_RPN_BBOX_GAIN)

    def fc(name, cout, cin, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((cout, cin)) * gain * np.sqrt(2.0 / cin)).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    fc("roi_heads.box.predictor.cls_score", ncls, 2048, C4_CLS_GAIN)
    fc("roi_heads.box.predictor.bbox_pred", nreg, 2048, C4_BBOX_GAIN)
    sd["roi_heads.box.predictor.cls_score.bias"][0] += C4_BG_BIAS
    sd["roi_heads.mask.predictor.conv5_mask.weight"] = (rng.standard_normal((2048, 256, 2, 2)) * np.sqrt(2.0 / 2048)).astype(np.float32)
    sd["roi_heads.mask.predictor.conv5_mask.bias"] = (rng.standard_normal(256) * 0.01).astype(np.float32)
    _conv_bias(rng, sd, "roi_heads.mask.predictor.mask_fcn_logits", ncls, 256, 1, gain=C4_MASK_LOGIT_GAIN)
    return sd if mask else _drop_mask_head(sd)


KEYPOINT_SEED_OFFSET = 7919   # the head's own generator: seed + this, so the trunk's tensors equal maskrcnn_state_dict's of the same seed


def keypointrcnn_state_dict(seed=1234, depth=50, conv_layers=(512,) * 8, num_keypoints=17):
    """[UPSTREAM-RECALL] maskrcnn-benchmark e2e_keypoint_rcnn_R_50/101_FPN state-dict names: the two-class box-only model
    (maskrcnn_state_dict(seed, depth, mask=False, num_classes=2), tensor for tensor) plus roi_heads.keypoint.feature_extractor.conv_fcn{1..}.{weight,bias}
    (3x3, 256 -> 512 -> ... -> 512) and roi_heads.keypoint.predictor.kps_score_lowres.{weight,bias}, the weight [512][17][4][4] as ConvTranspose2d stores it.
    The head is drawn from a generator of its own."""
    sd = maskrcnn_state_dict(seed, depth, mask=False, num_classes=2)
    rng = np.random.default_rng(seed + KEYPOINT_SEED_OFFSET)
    cin = 256
    for i, cout in enumerate(conv_layers, 1):
        _conv_bias(rng, sd, "roi_heads.keypoint.feature_extractor.conv_fcn%d" % i, int(cout), cin, 3)
        cin = int(cout)
    # He initialisation: a transposed convolution's output pixel sums 4 live taps x cin inputs
    sd["roi_heads.keypoint.predictor.kps_score_lowres.weight"] = (rng.standard_normal((cin, num_keypoints, 4, 4)) * np.sqrt(2.0 / (4 * cin))).astype(np.float32)
    sd["roi_heads.keypoint.predictor.kps_score_lowres.bias"] = (rng.standard_normal(num_keypoints) * 0.01).astype(np.float32)
    return sd


def random_maskrcnn_state_dict(cfg, seed=1234):
    """The seeded weights of `MODEL.WEIGHT random` for a MaskRCNNConfig: the generator of its body / norm, sized by MASK_ON, NUM_CLASSES and
    CLS_AGNOSTIC_BBOX_REG."""
    if getattr(cfg, "KEYPOINT_ON", False):   # Keypoint R-CNN: the two-class box-only trunk plus the keypoint head
        if int(cfg.NUM_CLASSES) != 2 or cfg.CLS_AGNOSTIC_BBOX_REG:
            raise ValueError("MODEL.KEYPOINT_ON: the seeded generator draws the upstream model, MODEL.ROI_BOX_HEAD.NUM_CLASSES 2 with per-class regression")
        return keypointrcnn_state_dict(seed, cfg.depth, cfg.KEYPOINT_CONV_LAYERS, cfg.NUM_KEYPOINTS)
    kw = dict(mask=bool(cfg.MASK_ON), num_classes=int(cfg.NUM_CLASSES), cls_agnostic=bool(cfg.CLS_AGNOSTIC_BBOX_REG))
    if cfg.is_c4:
        return maskrcnn_c4_state_dict(seed, **kw)
    if cfg.USE_GN:
        return maskrcnn_gn_state_dict(seed, cfg.depth, cfg.BOX_HEAD_STACKED_CONVS, cfg.BOX_HEAD_CONV_DIM, cfg.BOX_HEAD_MLP_DIM, **kw)
    return maskrcnn_state_dict(seed, cfg.depth, groups=int(getattr(cfg, "NUM_GROUPS", 1)), width_per_group=int(getattr(cfg, "WIDTH_PER_GROUP", 64)),
                               stage_with_dcn=tuple(getattr(cfg, "STAGE_WITH_DCN", (0, 0, 0, 0))), modulated=bool(getattr(cfg, "WITH_MODULATED_DCN", False)), **kw)


# Synthetic pose templates in the 64 x 64 align frame, COCO keypoint order (nose, eyes, ears, shoulders, elbows, wrists, hips, knees,
# ankles; left before right).  NOT upstream's templates.json: an upright pose with the left arm raised, its mirror with left and right
# swapped, and a crouch.  Weight 1 on every joint.
_POSE_UPRIGHT = [(32, 8), (34, 6), (30, 6), (36, 7), (28, 7), (40, 16), (24, 16), (45, 22), (21, 26), (46, 14), (20, 35), (37, 36), (27, 36),
                 (38, 47), (26, 47), (38, 58), (26, 58)]
_POSE_CROUCH = [(32, 16), (34, 14), (30, 14), (36, 15), (28, 15), (40, 24), (24, 24), (43, 32), (21, 32), (40, 38), (24, 38), (37, 40), (27, 40),
                (43, 48), (21, 48), (38, 58), (26, 58)]
_COCO_FLIP = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def pose_templates():
    up = np.array([(x, y, 1.0) for x, y in _POSE_UPRIGHT], np.float32)
    mirror = up[_COCO_FLIP].copy()
    mirror[:, 0] = 64.0 - mirror[:, 0]
    crouch = np.array([(x, y, 1.0) for x, y in _POSE_CROUCH], np.float32)
    return np.stack([up, mirror, crouch])


def pose2seg_state_dict(seed=1234, cat_skeleton=True, width=64, blocks=(3, 4, 6, 3), fpn_channels=256, seg_width=64, seg_blocks=(10, 1)):
    """Seeded synthetic Pose2Seg weights: a torchvision-form ResNet (backbone.conv1 / bn1 / layers.L.B.*), the FPN laterals and P2 output
    conv (fpn.lateral2..5, fpn.output2..5), the SegModule (segnet.conv1 / bn1, segnet.stage1.B.* ten bottlenecks, segnet.stage2.0.* one,
    segnet.conv_out 1x1 -> 2) and `pose_templates` [3][17][3] -- SYNTHETIC templates (pose_templates()), not upstream's templates.json.
    The defaults are the paper's widths; the tests use narrower ones (the engine reads every width from the weight shapes)."""
    rng = np.random.default_rng(seed)
    sd = {}

    def bneck(nm, cin, planes, proj):
        sd[nm + ".conv1.weight"] = _conv(rng, planes, cin, 1); _bn(rng, sd, nm + ".bn1", planes)
        sd[nm + ".conv2.weight"] = _conv(rng, planes, planes, 3); _bn(rng, sd, nm + ".bn2", planes)
        sd[nm + ".conv3.weight"] = _conv(rng, planes * 4, planes, 1); _bn(rng, sd, nm + ".bn3", planes * 4, 0.25)
        if proj:
            sd[nm + ".downsample.0.weight"] = _conv(rng, planes * 4, cin, 1)
            _bn(rng, sd, nm + ".downsample.1", planes * 4)

    sd["backbone.conv1.weight"] = _conv(rng, width, 3, 7)
    _bn(rng, sd, "backbone.bn1", width)
    cin = width
    for li, nb in enumerate(blocks):
        planes = width << li
        for b in range(nb):
            bneck("backbone.layers.%d.%d" % (li, b), cin, planes, b == 0)
            cin = planes * 4
    for l in range(4):
        _conv_bias(rng, sd, "fpn.lateral%d" % (l + 2), fpn_channels, (width * 4) << l, 1)
        _conv_bias(rng, sd, "fpn.output%d" % (l + 2), fpn_channels, fpn_channels, 3)
    cin = fpn_channels + (55 if cat_skeleton else 0)
    sd["segnet.conv1.weight"] = _conv(rng, seg_width, cin, 7)
    _bn(rng, sd, "segnet.bn1", seg_width)
    cin = seg_width
    for si, nb in enumerate(seg_blocks):
        for b in range(nb):
            bneck("segnet.stage%d.%d" % (si + 1, b), cin, seg_width, cin != seg_width * 4)
            cin = seg_width * 4
    _conv_bias(rng, sd, "segnet.conv_out", 2, cin, 1, bias_std=0.1)
    sd["pose_templates"] = pose_templates()
    return sd


def vit_random_state_dict(cfg, seed=1234, H=224, W=224):
    """Seeded random ViT weights in the timm names (isegmi.vit.ViTConfig): linear layers N(0, 1 / fan_in) (the blocks' output projections damped so the
    residual stream stays O(1) over the depth), LayerNorm weight U(0.5, 1.5) / bias N(0, 0.1), class token and position embedding N(0, 0.02^2) as
    published, the head with a gain that spreads the class probabilities."""
    rng = np.random.default_rng(seed)
    D, T = cfg.dim, cfg.tokens(H, W)

    def f(a):
        return np.asarray(a, np.float32)

    def linear(name, cout, cin, gain=1.0):
        sd[name + ".weight"] = f(rng.standard_normal((cout, cin)) * (gain / np.sqrt(cin)))
        sd[name + ".bias"] = f(rng.standard_normal(cout) * 0.02)

    def norm(name):
        sd[name + ".weight"] = f(rng.uniform(0.5, 1.5, D))
        sd[name + ".bias"] = f(rng.standard_normal(D) * 0.1)

    sd = {"cls_token": f(rng.standard_normal((1, 1, D)) * 0.02), "pos_embed": f(rng.standard_normal((1, T, D)) * 0.02)}
    k = 3 * cfg.patch * cfg.patch
    sd["patch_embed.proj.weight"] = f(rng.standard_normal((D, 3, cfg.patch, cfg.patch)) / np.sqrt(k))
    sd["patch_embed.proj.bias"] = f(rng.standard_normal(D) * 0.02)
    for i in range(cfg.depth):
        b = "blocks.%d." % i
        norm(b + "norm1")
        linear(b + "attn.qkv", 3 * D, D, 2.0)   # q, k of unit-ish variance: scores that spread over a few units, a softmax that is not flat
        linear(b + "attn.proj", D, D, 0.5)
        norm(b + "norm2")
        linear(b + "mlp.fc1", cfg.mlp_dim, D)
        linear(b + "mlp.fc2", D, cfg.mlp_dim, 0.5)
    norm("norm")
    linear("head", cfg.num_classes, D, 2.0)
    return sd
