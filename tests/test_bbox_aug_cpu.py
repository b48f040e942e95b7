"""Test-time box augmentation without a GPU: the view list, the config mapping with every acceptance and refusal, the reference
(tests/bbox_aug_ref.py) against the CPU oracle and against float64, and the crafted cases that tell the rules apart."""
import os

import numpy as np
import pytest

import bbox_aug_cases as bc
import bbox_aug_ref as br
from decision_cases import threshold_logits
from oracle import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
YAML = "e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml"


def _node(name, *kv):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", name))
    c.merge_from_list(list(kv))
    return c


# ------------------------------------------------------------------------------------------------------------------------ views
def test_views_order_and_sizes():
    from isegmi.config import to_bbox_aug_config
    from isegmi.maskrcnn import bbox_aug_engine_side, bbox_aug_views
    mc, aug = to_bbox_aug_config(_node(YAML))
    v = bbox_aug_views((480, 640), mc, aug)
    assert v == [(800, 1066, False), (800, 1066, True), (400, 533, False), (400, 533, True), (600, 800, False), (600, 800, True),
                 (1000, 1333, False), (1000, 1333, True), (1200, 1600, False), (1200, 1600, True)]
    # a 1 : 3 image: the identity view hits MAX_SIZE_TEST 1333 (short side round(1333 / 3) = 444, long side int(444 * 3)), the scales 1000 and 1200 hit
    # TEST.BBOX_AUG.MAX_SIZE 2000: short side round(2000 / 3) = 667, and get_size's truncating long side is int(667 * 3) = 2001 -- one over, as upstream's
    w = bbox_aug_views((300, 900), mc, aug)
    assert w[0] == (444, 1332, False) and w[2] == (400, 1200, False) and w[4] == (600, 1800, False) and w[6] == (667, 2001, False) and w[8] == (667, 2001, False)
    assert bbox_aug_engine_side(mc, aug) == 2016   # min(2000, ceil(1200 * 1333 / 800) = 2000), rounded up to 32
    # no flips, no scales: the identity view alone; flips off keep the scales' order
    import dataclasses
    assert bbox_aug_views((480, 640), mc, dataclasses.replace(aug, H_FLIP=False, SCALES=(), SCALE_H_FLIP=False)) == [(800, 1066, False)]
    assert bbox_aug_views((480, 640), mc, dataclasses.replace(aug, H_FLIP=False, SCALES=(1200, 400), SCALE_H_FLIP=False)) == \
        [(800, 1066, False), (1200, 1600, False), (400, 533, False)]
    assert bbox_aug_views((480, 640), mc, aug, min_size=96, max_size=160)[0] == (96, 128, False)


# ------------------------------------------------------------------------------------------------------------------------ config
def test_defaults_and_the_shipped_yaml():
    from isegmi.config import cfg, is_bbox_aug, to_bbox_aug_config
    a = cfg.TEST.BBOX_AUG
    assert (a.ENABLED, a.H_FLIP, tuple(a.SCALES), a.MAX_SIZE, a.SCALE_H_FLIP) == (False, False, (), 4000, False)   # [UPSTREAM-RECALL] defaults.py
    c = _node(YAML)
    assert is_bbox_aug(c) and not is_bbox_aug(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml"))
    mc, aug = to_bbox_aug_config(c)
    assert (aug.H_FLIP, aug.SCALES, aug.MAX_SIZE, aug.SCALE_H_FLIP, aug.POOL_CAP) == (True, (400, 600, 1000, 1200), 2000, True, 8192)
    assert not mc.MASK_ON and mc.NUM_CLASSES == 81 and mc.CONV_BODY == "R-50-FPN"


@pytest.mark.parametrize("name", ["e2e_faster_rcnn_R_101_FPN_1x.yaml", "e2e_faster_rcnn_X_101_32x8d_FPN_1x.yaml", "e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml",
                                  "e2e_faster_rcnn_dconv_R_50_FPN_1x.yaml"])
def test_every_box_only_fpn_body_is_accepted(name):
    from isegmi.config import to_bbox_aug_config
    mc, aug = to_bbox_aug_config(_node(name, "TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.SCALES", (400,), "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 256))
    assert aug.SCALES == (400,) and not aug.H_FLIP and aug.MAX_SIZE == 4000 and mc.NUM_CLASSES == 256


@pytest.mark.parametrize("yaml_name,kv,key", [
    ("e2e_mask_rcnn_R_50_FPN_1x.yaml", (), r"MODEL\.MASK_ON"),
    ("e2e_faster_rcnn_R_50_C4_1x.yaml", (), r"MODEL\.BACKBONE\.CONV_BODY"),
    ("retinanet_R-50-FPN_1x.yaml", (), r"MODEL\.RETINANET_ON"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 257), r"MODEL\.ROI_BOX_HEAD\.NUM_CLASSES"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("TEST.BBOX_AUG.SCALES", (400, 0)), r"TEST\.BBOX_AUG\.SCALES"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("TEST.BBOX_AUG.SCALES", (-400,)), r"TEST\.BBOX_AUG\.SCALES"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("TEST.BBOX_AUG.SCALES", (400.5,)), r"TEST\.BBOX_AUG\.SCALES"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("TEST.BBOX_AUG.SCALES", (400, 1200), "TEST.BBOX_AUG.MAX_SIZE", 1000), r"TEST\.BBOX_AUG\.MAX_SIZE"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("MODEL.RPN_ONLY", True), r"MODEL\.RPN_ONLY"),
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", ("MODEL.KEYPOINT_ON", True), r"MODEL\.KEYPOINT_ON"),
])
def test_refusals_name_their_key(yaml_name, kv, key):
    from isegmi.config import to_bbox_aug_config
    with pytest.raises(ValueError, match=key):
        to_bbox_aug_config(_node(yaml_name, "TEST.BBOX_AUG.ENABLED", True, *kv))


def test_command_line_text_overrides_map_like_the_yaml():
    """What `test_net ... KEY VALUE` leaves in the node: SCALES as the text of a tuple (parsed by merge_from_list), MAX_SIZE and the flags as plain text."""
    from isegmi.config import to_bbox_aug_config
    text = ["TEST.BBOX_AUG.ENABLED", "True", "TEST.BBOX_AUG.SCALES", "(64, 128)", "TEST.BBOX_AUG.MAX_SIZE", "224", "TEST.BBOX_AUG.H_FLIP", "True"]
    mc, aug = to_bbox_aug_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", *text))
    assert (aug.SCALES, aug.MAX_SIZE, aug.H_FLIP, aug.SCALE_H_FLIP) == ((64, 128), 224, True, False)
    for bad_key, bad in (("TEST.BBOX_AUG.MAX_SIZE", "224.5"), ("TEST.BBOX_AUG.MAX_SIZE", "-3"), ("TEST.BBOX_AUG.SCALES", "(64, 12.5)"), ("TEST.BBOX_AUG.SCALES", "64")):
        with pytest.raises(ValueError, match=bad_key.replace(".", r"\.")):
            to_bbox_aug_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", *(text + [bad_key, bad])))
    with pytest.raises(ValueError, match=r"MODEL\.RPN\.FPN_POST_NMS_TOP_N_TEST"):   # the candidate stage holds 1024 rows: refused before any engine exists
        to_bbox_aug_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", *(text + ["MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "2000"])))


def test_a_config_without_the_key_is_not_an_aug_config():
    from isegmi.config import to_bbox_aug_config
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG\.ENABLED"):
        to_bbox_aug_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml"))


def test_the_other_mappings_still_refuse_the_key_and_point_at_the_new_one():
    from isegmi.config import to_keypointrcnn_config, to_maskrcnn_config, to_retinanet_config
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG\.ENABLED.*to_bbox_aug_config"):
        to_maskrcnn_config(_node(YAML))
    kp = "e2e_keypoint_rcnn_R_50_FPN_1x.yaml"
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG\.ENABLED"):
        to_keypointrcnn_config(_node(kp, "TEST.BBOX_AUG.ENABLED", True))
    rn = "retinanet_R-50-FPN_1x.yaml"
    to_retinanet_config(_node(rn))   # the plain config still maps
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG\.ENABLED"):
        to_retinanet_config(_node(rn, "TEST.BBOX_AUG.ENABLED", True))


def test_predictor_refuses_what_the_engine_is_not_built_for():
    from isegmi.maskrcnn import BBoxAugConfig, MaskRCNNConfig
    from isegmi.predictor import COCODemo
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG"):
        COCODemo(MaskRCNNConfig(MASK_ON=True), state_dict={}, bbox_aug=BBoxAugConfig())
    with pytest.raises(ValueError, match=r"TEST\.BBOX_AUG"):
        COCODemo(MaskRCNNConfig(MASK_ON=False), state_dict={}, bbox_aug=BBoxAugConfig(), fp16=True)
    demo = COCODemo(MaskRCNNConfig(MASK_ON=False), state_dict={}, bbox_aug=BBoxAugConfig(SCALES=(400,)))
    from isegmi.predictor import inference
    with pytest.raises(ValueError, match=r"world=2.*TEST\.BBOX_AUG"):
        demo.engine = lambda bs=None: type("NoDevice", (), {"box_only": True, "H": 32, "W": 32})()   # inference() asks for the engine first; the refusal needs no device
        inference(demo, [np.zeros((8, 8, 3), np.uint8)], world=2, rank=0)


# ------------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_the_cpu_oracle_on_the_identity_view():
    """MaskRCNNRef on the tiny batch (canvas 128 x 160): its filter_results output equals the reference's candidates + merge of the identity view alone,
    fed with the oracle's own predictor rows and proposals."""
    from fasterrcnn_cases import full_state_dict, tiny_batch
    from oracle.maskrcnn_ref import MaskRCNNRef
    x, hw = tiny_batch()
    ref = MaskRCNNRef(full_state_dict())
    d = ref.forward(x, hw)[0]
    cls, reg, pr = ref.dbg["cls"][0], ref.dbg["reg"][0], d["proposals"]
    view = dict(logits=cls, regr=reg, props=pr, prop_cnt=len(pr), image_hw=hw[0])
    (b, s, lb), total, per_view = br.detect([view], 81, cap=100)
    print("tiny batch: proposals", len(pr), "candidates", total, "detections", len(s))
    assert total > 100 and len(s) == len(d["score"]) > 0
    assert np.array_equal(b, d["box"]) and np.array_equal(s, d["score"]) and np.array_equal(lb, d["label"])
    # index order too
    ref4 = ora.box_postprocess(cls, reg, pr, float(hw[0][1]), float(hw[0][0]), 0.05, 0.5, 100, 4, 100)
    got4 = br.detect([view], 81, cap=100, nms_flags=4)[0]
    assert all(np.array_equal(u, v) for u, v in zip(got4, ref4))


def test_flip_and_ratio_arithmetic_against_float64():
    """On exactly representable inputs (integers and halves, power-of-two ratios) the fp32 reference equals float64 arithmetic exactly."""
    rng = np.random.default_rng(0)
    for w in (100, 101, 1333):
        b = np.sort(rng.integers(0, 2 * w, (64, 2, 2)) / 2.0, axis=1).reshape(64, 4)   # (x_lo, y_lo, x_hi, y_hi)
        b = np.minimum(b, w - 1.0).astype(F32)   # x1 <= x2, y1 <= y2
        f = br.unflip(b, w)
        b64 = b.astype(np.float64)
        assert np.array_equal(f[:, 0].astype(np.float64), w - b64[:, 2] - 1) and np.array_equal(f[:, 2].astype(np.float64), w - b64[:, 0] - 1)
        assert np.array_equal(f[:, [1, 3]], b[:, [1, 3]]) and (f[:, 0] <= f[:, 2]).all()
        assert np.array_equal(br.unflip(f, w), b)   # an involution on these inputs
        for r in (1.0, 2.0, 0.5):
            assert np.array_equal(br.to_view0(f, (r, r)).astype(np.float64), f.astype(np.float64) * r)
    # the ratio is float32 of the double quotient, as BoxList.resize computes it
    rw, rh = br.view_ratios((800, 1066), (1200, 1600))
    assert rw == F32(1066.0 / 1600.0) and rh == F32(800.0 / 1200.0) and br.view_ratios((800, 1066), (800, 1066)) == (F32(1.0), F32(1.0))
    from isegmi.maskrcnn import BoxList
    bl = BoxList(np.array([[10, 20, 30, 40]], F32), (1600, 1200)).resize((1066, 800))
    assert np.array_equal(bl.bbox, br.to_view0(np.array([[10, 20, 30, 40]], F32), (rw, rh)))


# ------------------------------------------------------------------------------------------------------------------------ discrimination
def _cands(view, **kw):
    return br.candidates(view["logits"], view["regr"], view["props"], view["prop_cnt"], view["image_hw"], kw.pop("hflip", False),
                         view.get("ratios_wh", (1.0, 1.0)), 0.05, False, **kw)


@pytest.mark.parametrize("w_view", [100, 101])
def test_the_crafted_cases_tell_the_rules_apart(w_view):
    # the flip's -1: every mirrored box moves by one pixel without it
    v = bc.border_view(w_view)
    right, wrong = _cands(v, hflip=True)[0], _cands(v, hflip=True, wrong="no_minus_one")[0]
    assert right.shape == wrong.shape == (5, 4) and (wrong[:, [0, 2]] == right[:, [0, 2]] + 1).all()
    assert right[1, 0] == 0 and right[0, 2] == w_view - 1   # a box on one border lands on the other
    # clip and unflip in the other order: the mirror map is monotone and maps [0, w - 1] onto itself, so NO answer changes -- on the crafted boxes (two of
    # them clipped on both sides) and on random ones; the order that matters is clip before the rescale, which clip_order_view tells apart
    assert np.array_equal(_cands(v, hflip=True, wrong="flip_before_clip")[0], right)
    rng = np.random.default_rng(w_view)
    rv = dict(logits=np.tile(np.array([0.0, 3.0], F32), (256, 1)), regr=rng.normal(0, 4.0, (256, 8)).astype(F32), props=bc._props(rng, 256, w_view, 60.0),
              prop_cnt=256, image_hw=(60, w_view))
    assert np.array_equal(_cands(rv, hflip=True, wrong="flip_before_clip")[0], _cands(rv, hflip=True)[0])
    c = bc.clip_order_view()
    for flip in (False, True):
        a, b = _cands(c, hflip=flip)[0], _cands(c, hflip=flip, wrong="clip_last")[0]
        assert not np.array_equal(a, b) and a[0, 2 if not flip else 0] in (198.0, 0.0)
    assert _cands(c)[0][0, 2] == 198.0 and _cands(c, wrong="clip_last")[0][0, 2] == 99.0


def test_the_threshold_is_strict():
    rows = threshold_logits(ora.softmax, 0.05, 5, cls=2)
    v = dict(logits=np.stack([rows["pred"], rows["on"], rows["succ"]]), regr=np.zeros((3, 20), F32), props=np.tile(np.array([[5, 5, 30, 30]], F32), (3, 1)),
             prop_cnt=3, image_hw=(64, 64))
    is2 = lambda out: [int(r) for r in np.flatnonzero(out[2] == 2)]
    right, wrong = _cands(v), _cands(v, wrong="ge")
    assert len(right[1]) + 1 == len(wrong[1]) and (right[2] == 2).sum() == 1 and (wrong[2] == 2).sum() == 2
    assert F32(0.05) in wrong[1] and F32(0.05) not in right[1]


def test_rows_past_the_count_and_the_pool_cap():
    g = bc.generated(65, 81, "alternate", True)
    for n in range(4):
        b, s, lb = br.candidates(g["logits"][n], g["regr"][n], g["props"][n], g["cnt"][n], g["hw"][n], True, bc.RATIO_23, g["thr"], True)
        assert np.isfinite(b).all() and np.isfinite(s).all() and (len(s) > 0) == (g["cnt"][n] > 0)   # the NaN rows past the count are never looked at
        assert (np.diff(lb.astype(np.int64)) <= 0).sum() <= max(int(g["cnt"][n]) - 1, 0)                 # class ascending inside a proposal
    c = br.candidates(g["logits"][3], g["regr"][3], g["props"][3], 65, g["hw"][3], False, (1.0, 1.0), g["thr"], True)
    (pb, ps, pl), total = br.pool([c, c], cap=3000)
    assert total == 2 * len(c[1]) > 3000 and len(ps) == 3000 and np.array_equal(ps[: len(c[1])], c[1]) and np.array_equal(ps[len(c[1]):], c[1][: 3000 - len(c[1])])
    # equal scores order by slot: the earlier view's twin is visited first and survives the NMS
    twin = (c[0][:1], c[1][:1], c[2][:1])
    (mb, ms, ml) = br.merge(br.pool([twin, twin])[0], 81)
    assert len(ms) == 1
