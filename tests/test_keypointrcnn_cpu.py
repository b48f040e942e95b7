"""Keypoint R-CNN, the host side: the config mapping and its refusals, the weight generator and importer families, the transposed
convolution's packing against torch, the keypoint record block's layout, the json entry, and the numpy restatement of the decode (tests/keypoint_ref.py)
against torch's bicubic as a second opinion and on the crafted inputs of tests/keypoint_cases.py."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

import keypoint_cases as kc
import keypoint_ref as kr
from conftest import ROOT

YAMLS = (("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "R-50-FPN", 50), ("e2e_keypoint_rcnn_R_101_FPN_1x.yaml", "R-101-FPN", 101))


def _node(name="e2e_keypoint_rcnn_R_50_FPN_1x.yaml", *opts):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", name))
    for k, v in zip(opts[::2], opts[1::2]):
        c.merge_from_list([k, v])
    return c


@pytest.mark.parametrize("name,body,depth", YAMLS)
def test_keypoint_yamls_map(name, body, depth):
    from isegmi.config import is_keypoint_rcnn, is_retinanet, to_keypointrcnn_config
    c = _node(name)
    assert is_keypoint_rcnn(c) and not is_retinanet(c)
    mc = to_keypointrcnn_config(c)
    assert mc.KEYPOINT_ON is True and mc.MASK_ON is False and mc.NUM_CLASSES == 2 and mc.CLS_AGNOSTIC_BBOX_REG is False
    assert mc.CONV_BODY == body and mc.depth == depth and not mc.USE_GN and not mc.is_c4
    assert mc.KEYPOINT_CONV_LAYERS == (512,) * 8 and mc.NUM_KEYPOINTS == 17 and mc.det_cap == 100


def test_defaults_leave_every_existing_model_as_it_is():
    from isegmi.config import cfg, is_keypoint_rcnn, to_maskrcnn_config
    from isegmi.maskrcnn import MaskRCNNConfig
    d = MaskRCNNConfig()
    assert d.KEYPOINT_ON is False and d.KEYPOINT_CONV_LAYERS == (512,) * 8 and d.NUM_KEYPOINTS == 17
    c = cfg.clone()
    assert not is_keypoint_rcnn(c) and to_maskrcnn_config(c) == d
    k = c.MODEL.ROI_KEYPOINT_HEAD
    assert (k.FEATURE_EXTRACTOR, k.PREDICTOR) == ("KeypointRCNNFeatureExtractor", "KeypointRCNNPredictor")
    assert (k.POOLER_RESOLUTION, k.POOLER_SAMPLING_RATIO, k.RESOLUTION, k.NUM_CLASSES, k.SHARE_BOX_FEATURE_EXTRACTOR) == (14, 2, 56, 17, False)
    assert tuple(k.POOLER_SCALES) == (0.25, 0.125, 0.0625, 0.03125) and tuple(k.CONV_LAYERS) == (512,) * 8


def test_to_maskrcnn_config_still_refuses_keypoint_on_and_names_the_other_function():
    from isegmi.config import to_keypointrcnn_config, to_maskrcnn_config
    with pytest.raises(ValueError, match=r"MODEL\.KEYPOINT_ON.*to_keypointrcnn_config"):
        to_maskrcnn_config(_node())
    with pytest.raises(ValueError, match=r"MODEL\.KEYPOINT_ON.*to_maskrcnn_config"):
        to_keypointrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml"))


REFUSALS = (
    (("MODEL.MASK_ON", True), r"MODEL\.MASK_ON"),
    (("MODEL.BACKBONE.CONV_BODY", "R-50-C4"), r"MODEL\.BACKBONE\.CONV_BODY"),
    (("MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", True), r"MODEL\.ROI_KEYPOINT_HEAD\.SHARE_BOX_FEATURE_EXTRACTOR"),
    (("MODEL.ROI_KEYPOINT_HEAD.FEATURE_EXTRACTOR", "ResNet50Conv5ROIFeatureExtractor"), r"MODEL\.ROI_KEYPOINT_HEAD\.FEATURE_EXTRACTOR"),
    (("MODEL.ROI_KEYPOINT_HEAD.PREDICTOR", "Other"), r"MODEL\.ROI_KEYPOINT_HEAD\.PREDICTOR"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 7), r"MODEL\.ROI_KEYPOINT_HEAD\.POOLER_RESOLUTION"),
    (("MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 28), r"MODEL\.ROI_KEYPOINT_HEAD\.RESOLUTION"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", 0), r"MODEL\.ROI_KEYPOINT_HEAD\.POOLER_SAMPLING_RATIO"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", "(0.125, 0.0625, 0.03125, 0.015625)"), r"MODEL\.ROI_KEYPOINT_HEAD\.POOLER_SCALES"),
    (("MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", "()"), r"MODEL\.ROI_KEYPOINT_HEAD\.CONV_LAYERS"),
    (("MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", "(512, 500)"), r"MODEL\.ROI_KEYPOINT_HEAD\.CONV_LAYERS"),
    (("MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", 0), r"MODEL\.ROI_KEYPOINT_HEAD\.NUM_CLASSES"),
    (("MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", 33), r"MODEL\.ROI_KEYPOINT_HEAD\.NUM_CLASSES"),
    (("MODEL.RPN_ONLY", True), r"MODEL\.RPN_ONLY"),
    (("TEST.BBOX_AUG.ENABLED", True), r"TEST\.BBOX_AUG\.ENABLED"),
)


@pytest.mark.parametrize("opts,match", REFUSALS, ids=["%s=%s" % o for o, _ in REFUSALS])
def test_refusals_name_the_key(opts, match):
    from isegmi.config import to_keypointrcnn_config
    with pytest.raises(ValueError, match=match):
        to_keypointrcnn_config(_node("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", *opts))


def test_groupnorm_body_is_refused():
    from isegmi.config import to_keypointrcnn_config
    c = _node("e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml", "MODEL.KEYPOINT_ON", True)
    with pytest.raises(ValueError, match=r"MODEL\.KEYPOINT_ON with GroupNorm"):
        to_keypointrcnn_config(c)


def test_accepted_variations():
    from isegmi.config import to_keypointrcnn_config
    mc = to_keypointrcnn_config(_node("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", "(64, 96)", "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", 5))
    assert mc.KEYPOINT_CONV_LAYERS == (64, 96) and mc.NUM_KEYPOINTS == 5


# ---- weights
def _head_shapes(layers=(512,) * 8, nk=17):
    out, cin = {}, 256
    for i, c in enumerate(layers, 1):
        out["roi_heads.keypoint.feature_extractor.conv_fcn%d.weight" % i] = (c, cin, 3, 3)
        out["roi_heads.keypoint.feature_extractor.conv_fcn%d.bias" % i] = (c,)
        cin = c
    out["roi_heads.keypoint.predictor.kps_score_lowres.weight"] = (cin, nk, 4, 4)
    out["roi_heads.keypoint.predictor.kps_score_lowres.bias"] = (nk,)
    return out


def test_generator_key_set_shapes_and_untouched_trunk():
    from isegmi.weights import keypointrcnn_state_dict, maskrcnn_state_dict, random_maskrcnn_state_dict
    sd = keypointrcnn_state_dict(1234)
    trunk = maskrcnn_state_dict(1234, mask=False, num_classes=2)
    head = {k: v for k, v in sd.items() if k.startswith("roi_heads.keypoint.")}
    assert {k: v.shape for k, v in head.items()} == _head_shapes()
    assert set(sd) == set(trunk) | set(head) and not [k for k in sd if k.startswith("roi_heads.mask.")]
    assert all(v.dtype == np.float32 for v in sd.values())
    for k, v in trunk.items():
        assert np.array_equal(sd[k], v), k                                     # the head has a generator of its own
    again = keypointrcnn_state_dict(1234)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    other = keypointrcnn_state_dict(7, conv_layers=(64, 96), num_keypoints=5)
    assert {k: v.shape for k, v in other.items() if k.startswith("roi_heads.keypoint.")} == _head_shapes((64, 96), 5)
    assert sd["roi_heads.box.predictor.cls_score.weight"].shape[0] == 2 and sd["roi_heads.box.predictor.bbox_pred.weight"].shape[0] == 8
    from isegmi.config import to_keypointrcnn_config
    rnd = random_maskrcnn_state_dict(to_keypointrcnn_config(_node()), 1234)
    assert set(rnd) == set(sd) and all(np.array_equal(rnd[k], sd[k]) for k in sd)


def _importer():
    spec = importlib.util.spec_from_file_location("import_pth", os.path.join(ROOT, "tools", "import_pth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("family,depth", [("keypointrcnn_r50_fpn", 50), ("keypointrcnn_r101_fpn", 101)])
def test_importer_family_round_trip(family, depth):
    from isegmi.weights import keypointrcnn_state_dict
    mod = _importer()
    assert family in mod.FAMILIES
    exp = mod.expected_keys(family)
    assert {k: v for k, v in exp.items() if k.startswith("roi_heads.keypoint.")} == _head_shapes()
    assert exp["roi_heads.box.predictor.cls_score.weight"][0] == 2
    sd = keypointrcnn_state_dict(3, depth)
    out = mod.convert(dict(sd), family)
    assert set(out) == set(exp) and all(np.array_equal(out[k], sd[k]) for k in sd)
    short = {k: v for k, v in sd.items() if "kps_score_lowres" not in k}
    with pytest.raises(KeyError, match="kps_score_lowres"):
        mod.convert(short, family)
    with pytest.raises(ValueError, match="shape mismatch"):                     # a keypoint checkpoint is not an 81-class Faster R-CNN one
        mod.convert(dict(sd), "fasterrcnn_r50_fpn" if depth == 50 else "fasterrcnn_r101_fpn")
    c2 = {"conv1_w": np.zeros((64, 3, 7, 7), np.float32), "res_conv1_bn_s": np.ones(64, np.float32), "kps_score_lowres_w": np.zeros((512, 17, 4, 4), np.float32)}
    with pytest.raises(ValueError, match=family):                               # a Detectron pickle: the name mapping does not cover the head
        mod.convert(c2, family)


def test_engine_wrapper_refuses_before_any_device_is_touched():
    """KEYPOINT_ON against fp16, C4, GroupNorm, MASK_ON and a dict without / with the head: all raised in __init__ before the library is loaded."""
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import keypointrcnn_state_dict, maskrcnn_state_dict
    kcfg = dataclasses.replace(MaskRCNNConfig(), MASK_ON=False, NUM_CLASSES=2, KEYPOINT_ON=True)
    sd = {}   # no weights are needed for these refusals
    with pytest.raises(ValueError, match=r"KEYPOINT_ON.*fp16"):
        MaskRCNN(sd, 128, 160, cfg=kcfg, fp16=True)
    with pytest.raises(ValueError, match=r"KEYPOINT_ON.*C4"):
        MaskRCNN(sd, 128, 160, cfg=dataclasses.replace(MaskRCNNConfig.c4(), MASK_ON=False, KEYPOINT_ON=True))
    with pytest.raises(ValueError, match=r"KEYPOINT_ON.*GroupNorm"):
        MaskRCNN(sd, 128, 160, cfg=dataclasses.replace(kcfg, USE_GN=True, BOX_HEAD="FPNXconv1fcFeatureExtractor"))
    with pytest.raises(ValueError, match=r"KEYPOINT_ON.*MASK_ON"):
        MaskRCNN(sd, 128, 160, cfg=dataclasses.replace(kcfg, MASK_ON=True))
    box_sd = maskrcnn_state_dict(5, mask=False, num_classes=2)
    with pytest.raises(ValueError, match=r"MODEL\.KEYPOINT_ON is True.*kps_score_lowres"):
        MaskRCNN(box_sd, 128, 160, cfg=kcfg)
    with pytest.raises(ValueError, match=r"roi_heads\.keypoint\..*MODEL\.KEYPOINT_ON is False"):
        MaskRCNN(keypointrcnn_state_dict(5), 128, 160, cfg=dataclasses.replace(kcfg, KEYPOINT_ON=False))


# ---- the transposed convolution as one 3 x 3 convolution + pixel shuffle
def test_packed_deconv_equals_conv_transpose2d_in_fp64():
    """(Cin 8, K 17, 14 x 14): conv3x3(pad 1) with the packed weights, shuffled, against torch.nn.functional.conv_transpose2d(kernel 4, stride 2, padding 1), all in
    fp64; every parity has exactly four live taps."""
    import torch
    from conv_ref import conv2d_fp64
    from isegmi.maskrcnn import pack_keypoint_deconv
    rng = np.random.default_rng(0)
    cin, nk = 8, 17
    w = rng.standard_normal((cin, nk, 4, 4)).astype(np.float32)
    b = rng.standard_normal(nk).astype(np.float32)
    x = rng.standard_normal((3, 14, 14, cin)).astype(np.float32)
    w3, b4 = pack_keypoint_deconv(w, b)
    assert w3.shape == (4 * nk, 3, 3, cin) and w3.dtype == np.float32 and np.array_equal(b4, np.tile(b, 4))
    live = (np.abs(w3).sum(3) > 0).reshape(4, nk, 9)
    assert (live.sum(2) == 4).all()                                             # four live taps per parity and keypoint, five zero ones
    got = kr.shuffle(conv2d_fp64(x, w3, 1, 1, None, b4).astype(np.float64), nk)
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(w.astype(np.float64)),
                                                torch.from_numpy(b.astype(np.float64)), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    assert got.shape == want.shape == (3, 28, 28, nk)
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(kr.conv_transpose2d_fp64(x, w, b) - want).max() < 1e-12       # the definition the GPU test uses


# ---- record block and json
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("cap", [100, 7])
def test_keypoint_block_layout(n, cap):
    from isegmi.dist import coco_record_layout, unpack_coco_records
    secs, coff, total = coco_record_layout(n, cap, 2, False, 0, box_only=True, keypoints=17)
    assert list(secs) == ["status", "box", "count", "score", "label", "kpt", "kscore"]
    assert total == coff == kc.block_bytes(n, cap) and total % 8 == 0
    assert all(off % 8 == 0 for off, _, _, _ in secs.values())
    assert secs["kpt"][1:] == (n * cap * 17 * 12, np.float32, (n, cap, 17, 3)) and secs["kscore"][1:] == (n * cap * 17 * 4, np.float32, (n, cap, 17))
    box_secs, _, box_total = coco_record_layout(n, cap, 2, False, 0, box_only=True)                  # existing callers are untouched
    assert {k: secs[k] for k in box_secs} == box_secs and secs["kpt"][0] == box_total
    rng = np.random.default_rng(n)
    count = rng.integers(0, cap + 1, n).astype(np.int32)
    vals = [rng.standard_normal(s).astype(np.float32) for s in ((n, cap, 4), (n, cap), (n, cap, 17, 3), (n, cap, 17))]
    label = rng.integers(1, 2, (n, cap)).astype(np.int32)
    ratios = rng.uniform(0.5, 2.0, (n, 2)).astype(np.float32)
    buf = kr.pack_records(vals[0], count, vals[1], label, vals[2], vals[3], ratios, n)
    rec = unpack_coco_records(buf, n, cap, 2, box_only=True, keypoints=17)
    assert np.array_equal(rec["count"], count) and np.array_equal(rec["kscore"], vals[3]) and rec["overflow"] is None
    assert np.array_equal(rec["kpt"][..., 2], vals[2][..., 2]) and np.array_equal(rec["kpt"][..., 0], vals[2][..., 0] * ratios[:, 0, None, None])
    with pytest.raises(AssertionError):
        coco_record_layout(n, cap, 2, False, 0, box_only=False, keypoints=17)


def test_json_entry_form():
    from isegmi.coco import label_categories, maskrcnn_results, results_from_records
    from isegmi.dist import unpack_coco_records
    rng = np.random.default_rng(3)
    cap, n = 7, 2
    count = np.array([2, 0], np.int32)
    box = np.zeros((n, cap, 4), np.float32); box[0, :2] = [[10.5, 20.25, 30.0, 60.5], [1.0, 2.0, 3.0, 4.0]]
    score = np.zeros((n, cap), np.float32); score[0, :2] = [0.9, 0.25]
    label = np.zeros((n, cap), np.int32); label[0, :2] = 1
    kpt = np.zeros((n, cap, 17, 3), np.float32); kpt[0, :2] = rng.uniform(0, 60, (2, 17, 3)); kpt[0, :2, :, 2] = 1.0
    ks = np.zeros((n, cap, 17), np.float32); ks[0, :2] = rng.standard_normal((2, 17))
    rec = unpack_coco_records(kr.pack_records(box, count, score, label, kpt, ks, np.ones((n, 2), np.float32), n), n, cap, 2, box_only=True, keypoints=17)
    cats = label_categories(2)
    assert cats == [None, 1]
    res = results_from_records(rec, [41, 42], [(100, 100), (100, 100)], 2, cap, categories=cats)
    assert len(res) == 2 and [d["image_id"] for d in res] == [41, 41]                                # the empty image: no entries
    d = res[0]
    assert sorted(d) == ["bbox", "category_id", "image_id", "keypoints", "score"] and d["category_id"] == 1
    assert d["bbox"] == [10.5, 20.25, 30.0 - 10.5 + 1.0, 60.5 - 20.25 + 1.0] and d["score"] == float(np.float32(0.9))
    assert len(d["keypoints"]) == 51 and d["keypoints"][2::3] == [1.0] * 17
    assert d["keypoints"] == kpt[0, 0].astype(np.float64).reshape(-1).tolist()
    assert res == maskrcnn_results(41, box[0, :2], score[0, :2], label[0, :2], categories=cats, keypoints=kpt[0, :2])
    import json
    assert json.loads(json.dumps(res)) == res


def test_boxlist_resize_scales_keypoints():
    from isegmi.maskrcnn import BoxList
    bl = BoxList([[1, 2, 3, 4]], (100, 50))
    kp = np.array([[[10.0, 20.0, 1.0], [30.5, 40.25, 1.0]]], np.float32)
    bl.add_field("keypoints", kp); bl.add_field("keypoint_logits", np.array([[3.0, -1.0]], np.float32))
    out = bl.resize((250, 75))
    rw, rh = np.float32(2.5), np.float32(1.5)
    assert np.array_equal(out.get_field("keypoints"), kp * np.array([rw, rh, 1.0], np.float32)) and out.get_field("keypoints").dtype == np.float32
    assert np.array_equal(out.get_field("keypoint_logits"), bl.get_field("keypoint_logits")) and np.array_equal(kp[0, 0], [10.0, 20.0, 1.0])
    assert np.array_equal(out[np.array([0])].get_field("keypoints"), out.get_field("keypoints"))


def test_demo_draws_a_dot_per_keypoint_above_the_threshold():
    from isegmi.maskrcnn import BoxList
    from isegmi.predictor import COCODemo
    demo = COCODemo.__new__(COCODemo)
    bl = BoxList([[5, 5, 50, 50]], (64, 64))
    kp = np.zeros((1, 17, 3), np.float32); kp[0, :, 0] = 10 + 2 * np.arange(17); kp[0, :, 1] = 30; kp[0, :, 2] = 1
    logits = np.full((1, 17), 1.9, np.float32); logits[0, 4] = 2.5
    bl.add_field("keypoints", kp); bl.add_field("keypoint_logits", logits)
    img = np.zeros((64, 64, 3), np.uint8)
    demo.overlay_keypoints(img, bl)
    ys, xs = np.nonzero(img.any(2))
    assert ys.min() == 28 and ys.max() == 32 and xs.min() == 16 and xs.max() == 20                   # only keypoint 4 (x = 18): logit > 2


# ---- the restatement of the decode
def test_restatement_agrees_with_torch_bicubic():
    """keypoint_ref.resize_bicubic against torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the smooth-peak maps (seed 0, 17 channels)
    at the nine output sizes.  The two sum in different orders, so values are held to 16 * 2^-23 * 1.375^2 * max|m| (1.375 = the largest sum of |w| of the
    cubic weights, at t = 1/2); the arg-max must agree on every map, and no map may have an exact tie for its maximum (then "first" would be a second
    condition on torch).  Measured here: largest difference 7.2e-6 at max|m| = 8.1 (bound 2.9e-5); arg-max equal on 153 of 153 maps; no tie."""
    import torch
    maps = kc.smooth_peak_maps(0)
    assert maps.shape == (56, 56, 17)
    bound = 16 * 2.0 ** -23 * 1.375 ** 2 * float(np.abs(maps).max())
    t = torch.from_numpy(np.ascontiguousarray(maps.transpose(2, 0, 1)))[None]
    agree = worst = 0
    for hc, wc in kc.TORCH_SIZES:
        want = torch.nn.functional.interpolate(t, size=(hc, wc), mode="bicubic", align_corners=False)[0].numpy()
        for k in range(17):
            got = kr.resize_bicubic(maps[:, :, k], hc, wc)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want[k]).max()))
            assert int((got == got.max()).sum()) == 1, (hc, wc, k)
            agree += int(np.argmax(got) == np.argmax(want[k]))
    print("restatement vs torch bicubic: max |diff| %.3g (bound %.3g), arg-max equal on %d of %d maps" % (worst, bound, agree, 17 * len(kc.TORCH_SIZES)))
    assert worst <= bound
    assert agree == 17 * len(kc.TORCH_SIZES)


def test_identity_size_is_the_identity():
    maps = kc.smooth_peak_maps(4)
    for k in (0, 16):
        assert np.array_equal(kr.resize_bicubic(maps[:, :, k], 56, 56), maps[:, :, k])
    box, m = kc.detections()["identity"]
    kpt, score, pos = kr.decode_one(m, box)
    for k in range(17):
        p = int(np.argmax(m[:, :, k]))
        assert pos[k] == p and score[k] == m[:, :, k].reshape(-1)[p]
        assert np.array_equal(kpt[k], np.array([p % 56 + 0.5 + 7.5, p // 56 + 0.5 + 9.25, 1.0], np.float32))


def test_cubic_weights():
    idx, w, s = kr.cubic_taps(112, 56)
    assert w.dtype == np.float32 and np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 1e-6
    assert idx.min() == 0 and idx.max() == 55 and (idx[0] == [0, 0, 0, 1]).all() and (idx[-1] == [54, 55, 55, 55]).all()
    _, w1, _ = kr.cubic_taps(1, 56)                                             # t = 1/2: (-0.09375, 0.59375, 0.59375, -0.09375), sum of |w| 1.375
    assert np.array_equal(w1[0], np.array([-0.09375, 0.59375, 0.59375, -0.09375], np.float32)) and np.abs(w1).sum() == 1.375


def test_crafted_inputs_discriminate():
    """The tie case really has two equal maxima in the restatement (and the later one in row-major order is further LEFT, so a column-major or a last-wins
    scan answers differently); the border case's maximum lies where the vertical taps are clamped; the last case's maximum is the last position; the
    all-zero maps answer position 0; and boxes and per-channel peaks are what the kernel test says they are."""
    d = kc.detections()
    box, m = d["tie"]
    w, h, wc, hc = kr.box_sizes(box)
    assert (wc, hc) == (112, 112)
    firsts = set()
    for k in range(17):
        r = kr.resize_bicubic(m[:, :, k], hc, wc)
        ys, xs = np.nonzero(r == r.max())
        assert len(ys) == 2 and ys[0] < ys[1] and xs[0] > xs[1], (k, ys, xs)
        assert (ys[1] - ys[0], xs[1] - xs[0]) == (20, -40)                         # (10, -20) source pixels at x2
        assert int(np.argmax(r)) == ys[0] * wc + xs[0] and int(np.argmax(r.T)) == xs[1] * hc + ys[1]   # a column-major scan finds the other one
        firsts.add((int(ys[0]), int(xs[0])))
    assert len(firsts) > 8                                                          # a different position per channel
    box, m = d["border"]
    _, _, wc, hc = kr.box_sizes(box)
    assert (wc, hc) == (168, 168)
    _, _, s = kr.cubic_taps(hc, 56)
    _, _, pos = kr.decode_one(m, box)
    assert ((pos // wc) < 3).all() and (s[pos // wc] - 1 < 0).all() and len(set((pos % wc).tolist())) == 17
    box, m = d["last"]
    _, _, wc, hc = kr.box_sizes(box)
    _, _, pos = kr.decode_one(m, box)
    assert (wc, hc) == (112, 84) and (pos == wc * hc - 1).all()
    box, m = d["zero"]
    kpt, score, pos = kr.decode_one(m, box)
    assert (pos == 0).all() and not score.any()
    assert kr.box_sizes(d["tiny"][0])[2:] == (1, 1) and kr.box_sizes(d["1x57"][0])[2:] == (1, 57) and kr.box_sizes(d["canvas"][0])[2:] == (1344, 800)
    w, h, wc, hc = kr.box_sizes(d["55.5x56.25"][0])
    assert (float(w), float(h), wc, hc) == (55.5, 56.25, 56, 57) and w / np.float32(wc) < 1
    w, h, wc, hc = kr.box_sizes(d["identity"][0])
    assert (float(w), float(h), wc, hc) == (56.0, 56.0, 56, 56)


def test_decode_batches_are_what_the_gpu_test_needs():
    heat, boxes, count, kpt, ks = kc.decode_batch(7)
    assert count.tolist() == [7, 0, 2] and not kpt[1].any() and not ks[1].any() and not kpt[2, 2:].any()
    assert np.isnan(heat[7:14]).all() and (kpt[0, :, :, 2] == 1).all() and np.isfinite(kpt).all() and np.isfinite(ks).all()
    assert kc.decode_batch(1)[2].tolist() == [1, 0] and kc.decode_batch(100)[2].tolist() == [37]
