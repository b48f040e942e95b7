"""The RetinaNet engine end to end against tests/retinanet_ref.py, bit for bit: pyramid, every level's selected list, final detections; canvas changes on
one engine, a partly filled batch, an empty result, a Mask R-CNN engine next to it, towers of 1 and 3 layers, a batch of three, the tail's parameters
changed on a live engine, and the refusals."""
import dataclasses

import numpy as np
import pytest

import retinanet_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(ffi):
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    m = RetinaNet(rc.state_dict(), 256, 352, RetinaNetConfig(DETECTIONS_CAP=128), max_batch=2)
    yield m
    m.close()


def test_reference_exercises_the_tail():
    """From the reference alone: the seeded weights reach every case of the tail on the small canvas."""
    x, hw, ref, dets = rc.reference("small", cap=128)
    assert [p.shape[1:3] for p in ref.feats["P"]] == [(32, 44), (16, 22), (8, 11), (4, 6), (2, 3)]
    from oracle import ora
    cands = [[int((ora.map_f32(lg[n], 1) > np.float32(0.05)).sum()) for n in range(2)] for lg in ref.feats["logits"]]
    flat = [c for lv in cands for c in lv]
    assert any(c > 1000 for c in flat), cands
    assert any(1 <= c <= 999 for c in flat), cands
    assert max(ref.feats["totals"]) > 100, ref.feats["totals"]
    assert all(len(set(d["label"].tolist())) >= 3 for d in dets), [set(d["label"].tolist()) for d in dets]


def test_small_canvas(model):
    x, hw, ref, dets = rc.reference("small", cap=128)
    preds = model(x, hw)
    rc.assert_forward_equal(model, ref, 2)
    rc.assert_dets_equal(preds, dets)


def test_canvas_changes_on_one_engine(model):
    """128 x 160 (P7 is 1 x 2) after the large canvas, then the large one again: anchors are laid out anew, results unchanged."""
    x, hw, ref, dets = rc.reference("small", cap=128)
    xt, hwt, reft, detst = rc.reference("tiny", cap=128)
    assert reft.feats["P"][4].shape[1:3] == (1, 2)
    rc.assert_dets_equal(model(x, hw), dets)
    predt = model(xt, hwt)
    rc.assert_forward_equal(model, reft, 1)
    rc.assert_dets_equal(predt, detst)
    assert sum(len(d["score"]) for d in detst) > 0
    rc.assert_dets_equal(model(x, hw), dets)
    rc.assert_forward_equal(model, ref, 2, features=False)


def test_one_image_in_an_engine_for_two(model):
    x, hw, ref, dets = rc.reference("first", cap=128)
    preds = model(x, hw)
    rc.assert_forward_equal(model, ref, 1)
    rc.assert_dets_equal(preds, dets)


def test_nothing_passes(ffi):
    from isegmi.retinanet import RetinaNet
    from isegmi.weights import retinanet_state_dict
    x, hw, _, _ = rc.reference("small", cap=128)
    m = RetinaNet(retinanet_state_dict(rc.SEED, cls_bias=-30.0), 256, 352, max_batch=2)
    try:
        preds = m(x, hw)
        assert [len(p) for p in preds] == [0, 0]
        assert all(p.bbox.shape == (0, 4) and p.get_field("scores").shape == (0,) and p.get_field("labels").shape == (0,) for p in preds)
        assert not m.fetch("retina.sel_cnt", 2).any()
    finally:
        m.close()


def test_next_to_a_maskrcnn_engine(model):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw, ref, dets = rc.reference("small", cap=128)
    mr = MaskRCNN(maskrcnn_state_dict(rc.SEED), 256, 352, max_batch=2)
    try:
        first = mr(x, hw)
        for _ in range(2):
            rc.assert_dets_equal(model(x, hw), dets)
            again = mr(x, hw)
            for a, b in zip(first, again):
                assert np.array_equal(rc.bits(a.bbox), rc.bits(b.bbox)) and np.array_equal(rc.bits(a.get_field("scores")), rc.bits(b.get_field("scores")))
                assert np.array_equal(a.get_field("mask"), b.get_field("mask"))
    finally:
        mr.close()


def test_forks_reach_the_tail(ffi):
    """nms_ge + plain areas + index order through the engine parameters."""
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    x, hw, ref, dets = rc.reference("small", cap=128, nms_flags=7)
    m = RetinaNet(rc.state_dict(), 256, 352, RetinaNetConfig(DETECTIONS_CAP=128, NMS_GE=1, NMS_PLUS_ONE=0, NMS_OUTPUT_ORDER="index"), max_batch=2)
    try:
        rc.assert_dets_equal(m(x, hw), dets)
    finally:
        m.close()


@pytest.mark.parametrize("num_convs", [1, 3])
def test_other_tower_depths(ffi, num_convs):
    """retina_num_convs 1 and 3: the towers' ping-pong ends in the other buffer than at 4 (and 1 never writes the second one)."""
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    x, hw, ref, dets4 = rc.reference("small", cap=128)
    sel, dets = rc.tail("small", num_convs)
    assert any(not np.array_equal(a["score"], b["score"]) for a, b in zip(dets, dets4))      # the depth reaches the result
    m = RetinaNet(rc.state_dict_convs(num_convs), 256, 352, RetinaNetConfig(DETECTIONS_CAP=128, NUM_CONVS=num_convs), max_batch=2)
    try:
        preds = m(x, hw)
        logits = rc.heads("small", num_convs)[0]
        for l in range(5):
            assert np.array_equal(rc.bits(m.fetch("retina.logits%d" % l, 2)), rc.bits(logits[l])), l
        rc.assert_selected_equal(m, sel, 2)
        rc.assert_dets_equal(preds, dets)
    finally:
        m.close()


def test_three_images_then_one(ffi):
    """max_batch 3: three images in one forward, then one image on the same engine -- nothing of the images 1 and 2 of the step before reaches it."""
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    x, hw, ref, dets = rc.reference("small", cap=128)
    x3, hw3, ref3, dets3 = rc.three()
    assert np.array_equal(rc.bits(x3[:2]), rc.bits(x)) and np.array_equal(hw3[:2], hw) and x3.shape == (3, 256, 352, 3)
    x1, hw1, ref1, dets1 = rc.reference("first", cap=128)
    assert len({len(d["score"]) for d in dets + dets3}) > 1 or not np.array_equal(dets[0]["score"], dets3[0]["score"])
    m = RetinaNet(rc.state_dict(), 256, 352, RetinaNetConfig(DETECTIONS_CAP=128), max_batch=3)
    try:
        preds = m(x3, hw3)
        rc.assert_selected_equal(m, ref.feats["sel"], 2)
        rc.assert_selected_equal(m, ref3.feats["sel"], 1, first=2)
        rc.assert_dets_equal(preds, dets + dets3)
        preds = m(x1, hw1)
        assert len(preds) == 1
        rc.assert_forward_equal(m, ref1, 1)
        rc.assert_dets_equal(preds, dets1)
        rc.assert_dets_equal(m(x3, hw3), dets + dets3)
    finally:
        m.close()


def test_tail_parameters_change_on_a_live_engine(model):
    """Each tail parameter changed and changed back on one engine: top_n alters the row stride of retina.sel_* / retina.cand_* and the workspaces' sizes."""
    x, hw, ref, dets = rc.reference("small", cap=128)
    rc.assert_dets_equal(model(x, hw), dets)
    seen = [[len(d["score"]) for d in dets]]
    for name, kw, values, back in (("retina_pre_nms_top_n", "top_n", (1024, 100), 1000), ("retina_inference_th", "thr", (0.5, 0.0), 0.05),
                                   ("retina_nms_th", "nms_thr", (0.6,), 0.4), ("detections_per_img", "det_per_img", (10,), 100)):
        try:
            for v in values:
                model.set_param(name, float(v))
                sel, want = rc.tail("small", **{kw: v})
                preds = model(x, hw)
                rc.assert_selected_equal(model, sel, 2)
                rc.assert_dets_equal(preds, want)
                assert any(not np.array_equal(a["score"], b["score"]) for a, b in zip(want, dets)) or \
                    any(len(sel[l][i][1]) != len(ref.feats["sel"][l][i][1]) for l in range(5) for i in range(2)), (name, v)     # the value reaches the lists or the result
                seen.append([len(d["score"]) for d in want])
        finally:
            model.set_param(name, float(back))
        preds = model(x, hw)
        rc.assert_forward_equal(model, ref, 2, features=False)
        rc.assert_dets_equal(preds, dets)
    assert len({tuple(s) for s in seen}) > 2, seen


def test_refusals(ffi, model):
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    with pytest.raises(ValueError, match="fp16"):
        RetinaNet(rc.state_dict(), 256, 352, fp16=True)
    with pytest.raises(ValueError, match="graph"):
        RetinaNet(rc.state_dict(), 256, 352, graph=True)
    with pytest.raises(ValueError, match="PRE_NMS_TOP_N"):
        RetinaNet(rc.state_dict(), 256, 352, dataclasses.replace(RetinaNetConfig(), PRE_NMS_TOP_N=1025))
    with pytest.raises(ValueError, match="five levels"):
        RetinaNet(rc.state_dict(), 256, 352, dataclasses.replace(RetinaNetConfig(), ANCHOR_STRIDES=(8, 16, 32, 64), ANCHOR_SIZES=(32, 64, 128, 256)))
    x, hw, ref, dets = rc.reference("small", cap=128)
    for name, bad, good in (("graph", 1.0, 0.0), ("fp16", 1.0, 0.0), ("retina_levels", 4.0, 5.0), ("retina_pre_nms_top_n", 2000.0, 1000.0)):
        model.set_param(name, bad)
        try:
            with pytest.raises(ffi.IsegmiError, match=name):
                model(x, hw)
        finally:
            model.set_param(name, good)
    rc.assert_dets_equal(model(x, hw), dets)


def test_cocodemo_and_inference_write_bbox_results(ffi, tmp_path):
    """COCODemo(cfg) with RETINANET_ON builds the RetinaNet engine; inference() on three small images (two canvases, bs = 2): bbox-only COCO records that
    equal the direct forward's, image by image."""
    import json
    import os
    from conftest import ROOT, smooth_field
    from isegmi.coco import maskrcnn_results
    from isegmi.config import cfg
    from isegmi.predictor import COCODemo, inference
    from isegmi.retinanet import RetinaNet
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "retinanet_R-50-FPN_1x.yaml"))
    rng = np.random.default_rng(41)
    shapes = [(150, 200), (200, 150), (150, 200)]
    images = [rng.integers(0, 256, (150, 200, 3)).astype(np.uint8), np.ascontiguousarray(smooth_field(7, 200, 150), np.uint8), rng.integers(0, 256, (150, 200, 3)).astype(np.uint8)]
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, state_dict=rc.state_dict(), max_image_size=320, max_batch=2)
    try:
        assert demo.is_retinanet and isinstance(demo.engine(), RetinaNet)
        direct = []
        for i, im in enumerate(images):
            p = demo.compute_prediction(im)
            assert not p.has_field("mask") and p.size == (im.shape[1], im.shape[0])
            direct += maskrcnn_results(10 + i, p.bbox, p.get_field("scores"), p.get_field("labels"))
        assert len(direct) > 20
        st = {}
        res = inference(demo, images, image_ids=[10, 11, 12], batch_size=2, stats=st)
        assert st["steps"] == 2 and st["images"] == 3
        lazy = inference(demo, lambda i: images[i], image_ids=[10, 11, 12], batch_size=1, sizes=shapes, workers=0)
        path = tmp_path / "bbox.json"
        path.write_text(json.dumps(res))
        back = json.loads(path.read_text())
        assert all("segmentation" not in d and len(d["bbox"]) == 4 for d in back)
        assert res == direct and lazy == direct
        out = demo.run_on_opencv_image(images[0])
        assert out.shape == images[0].shape and out.dtype == np.uint8
        with pytest.raises(ValueError, match="world"):
            inference(demo, images, world=2)
    finally:
        demo.close()
