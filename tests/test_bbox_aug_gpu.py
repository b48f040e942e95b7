"""Test-time box augmentation on the HIP engine (TEST.BBOX_AUG), bit for bit: six views (identity, two scales, every mirror image) of two
images of different sizes against tests/bbox_aug_ref.py fed with the PLAIN engine's own predictor rows and proposals of every view; the degenerate
config against the plain forward; plain forwards around an augmented pass; the overflow; the refusals; COCODemo, inference() and test_net.

INPUT.MIN_SIZE_TEST 96, MAX_SIZE_TEST 160, SCALES (64, 128), MAX_SIZE 224.  81 classes, SCORE_THRESH 0.04 and FPN_POST_NMS_TOP_N_TEST 300 were chosen with
the CPU oracle so that each image's pool holds several hundred candidates (far below 8192) and every view keeps detections through the merge; the central
test asserts both from the reference's side."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

import bbox_aug_ref as br
import fasterrcnn_cases as fc
from conftest import ROOT, smooth_field

pytestmark = pytest.mark.gpu
F32 = np.float32
MIN_SIZE, MAX_SIZE = 96, 160
OVERRIDES = ["INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE, "TEST.BBOX_AUG.SCALES", (64, 128), "TEST.BBOX_AUG.MAX_SIZE", 224,
             "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 300, "MODEL.ROI_HEADS.SCORE_THRESH", 0.04]


@functools.lru_cache(maxsize=None)
def images():
    out = [np.ascontiguousarray(smooth_field(3, 150, 200), np.uint8), np.ascontiguousarray(smooth_field(7, 210, 150), np.uint8),
           np.ascontiguousarray(smooth_field(11, 150, 200), np.uint8)]
    for im in out:
        im.setflags(write=False)
    return out


def node():
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml"))
    c.merge_from_list(OVERRIDES)
    return c


@functools.lru_cache(maxsize=None)
def configs():
    from isegmi.config import to_bbox_aug_config
    return to_bbox_aug_config(node())


@functools.lru_cache(maxsize=None)
def state_dict():
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(1234, mask=False)


@pytest.fixture(scope="module")
def model(ffi):
    from isegmi.maskrcnn import MaskRCNN, bbox_aug_engine_side
    mc, aug = configs()
    side = bbox_aug_engine_side(mc, aug)
    assert side == 224   # min(224, ceil(128 * 160 / 96) = 214) rounded up to 32
    m = MaskRCNN(state_dict(), side, side, cfg=mc, max_batch=2)
    yield m
    m.close()


def plain(model, resized):
    n = model.upload_u8(resized)
    model.forward_device(n); model.sync()
    return fc.fetch_dets(model, n)


def resized_views(ims):
    """-> [(resized images, hflip)] per view, in the view order, the mirror images made on the host"""
    from isegmi.transforms import maskrcnn_resize_u8
    mc, aug = configs()
    out = []
    for mn, mx, flip in [(MIN_SIZE, MAX_SIZE, aug.H_FLIP)] + [(s, aug.MAX_SIZE, aug.SCALE_H_FLIP) for s in aug.SCALES]:
        rs = [maskrcnn_resize_u8(im, mn, mx) for im in ims]
        out.append((rs, False))
        if flip:
            out.append(([np.ascontiguousarray(r[:, ::-1]) for r in rs], True))
    return out


def test_degenerate_aug_config_equals_the_plain_forward(model):
    from isegmi.maskrcnn import BBoxAugConfig
    from isegmi.transforms import maskrcnn_resize_u8
    ims = images()[:2]
    want = plain(model, [maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in ims])
    out = model.detect_aug(ims, BBoxAugConfig())
    got = fc.fetch_dets(model, 2)
    fc.assert_same_dets(got, want, "one view")
    assert int(want["det.count"].min()) > 0
    for n in range(2):
        assert np.array_equal(out[n].bbox, want["det.box"][n]) and out[n].size == (int(model._hw[n, 1]), int(model._hw[n, 0]))


def test_six_views_equal_the_reference_on_the_plain_engines_rows(model):
    from isegmi.maskrcnn import bbox_aug_views
    mc, aug = configs()
    ims = images()[:2]
    assert [v[2] for v in bbox_aug_views(ims[0].shape[:2], mc, aug)] == [False, True] * 3
    ncls, R = mc.NUM_CLASSES, mc.RPN_FPN_POST_NMS_TOP_N_TEST
    views = [[], []]
    hw0 = None
    for rs, hflip in resized_views(ims):
        plain(model, rs)
        hw = np.array([r.shape[:2] for r in rs], np.int32)
        hw0 = hw if hw0 is None else hw0
        cb = model.fetch("box.cls_bbox")[: 2 * R].reshape(2, R, 5 * ncls)
        props, pc = model.fetch("proposals", 2), model.fetch("proposal_count", 2)
        for n in range(2):
            views[n].append(dict(logits=cb[n, :, :ncls].copy(), regr=cb[n, :, ncls:].copy(), props=props[n].copy(), prop_cnt=int(pc[n]), image_hw=hw[n], hflip=hflip,
                                 ratios_wh=br.view_ratios(hw0[n], hw[n])))
    assert len(views[0]) == 6
    model.detect_aug(ims, aug)
    got = fc.fetch_dets(model, 2)
    totals = model.fetch("aug.pool_total", 2)
    for n in range(2):
        (b, s, lb), total, per_view = br.detect(views[n], ncls, thr=mc.ROI_SCORE_THRESH, nms_thr=mc.ROI_NMS, det_per_img=mc.DETECTIONS_PER_IMG, cap=mc.det_cap)
        # which view every surviving detection came from: its first slot in the pool (the NMS visits the earlier slot of equals first)
        cands = [br.candidates(v["logits"], v["regr"], v["props"], v["prop_cnt"], v["image_hw"], v["hflip"], v["ratios_wh"], mc.ROI_SCORE_THRESH) for v in views[n]]
        (pb, ps, pl), _ = br.pool(cands)
        edges = np.cumsum([0] + per_view)
        surv = np.zeros(6, int)
        for i in range(len(s)):
            slot = np.flatnonzero((ps == s[i]) & (pl == lb[i]) & (pb == b[i]).all(1))[0]
            surv[np.searchsorted(edges, slot, side="right") - 1] += 1
        print("image", n, "pool", total, "per view", per_view, "detections", len(s), "survivors per view", surv.tolist())
        assert 300 <= total < 8192 and int(totals[n]) == total
        assert (surv > 0).all(), surv
        assert got["det.count"][n] == len(s)
        assert np.array_equal(got["det.label"][n], lb) and np.array_equal(got["det.score"][n].view(np.uint32), s.view(np.uint32))
        assert np.array_equal(got["det.box"][n].view(np.uint32), b.view(np.uint32))
    assert np.array_equal(model._hw, hw0)   # the engine's current image sizes are view 0's again


def test_plain_forward_is_unchanged_by_an_aug_sequence(model):
    from isegmi.transforms import maskrcnn_resize_u8
    mc, aug = configs()
    rs = [maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in images()[:2]]
    before = plain(model, rs)
    model.detect_aug(images()[:2], aug)
    after = plain(model, rs)
    fc.assert_same_dets(before, after, "plain forward around an augmented pass")
    other = plain(model, [maskrcnn_resize_u8(images()[2], 128, 224)])   # another canvas right behind it
    assert other["det.count"][0] > 0


def test_a_small_pool_raises_and_names_the_cap(model):
    from isegmi.maskrcnn import BBoxAugOverflow
    mc, aug = configs()
    with pytest.raises(BBoxAugOverflow, match=r"POOL_CAP holds 64") as ei:
        model.detect_aug(images()[:2], dataclasses.replace(aug, POOL_CAP=64))
    total = model.fetch("aug.pool_total", 2)
    assert str(int(total.max())) in str(ei.value) and (model.fetch("aug.pool_cnt", 2) == 64).all()
    out = model.detect_aug(images()[:2], aug)   # the next pass starts from an empty pool
    assert len(out[0]) > 0 and (model.fetch("aug.pool_total", 2) == total).all()


def test_engine_refusals_by_name(ffi, model):
    L = ffi.lib()

    def refused(word, cap=8192, m=model):
        assert L.isegmi_maskrcnn_aug_begin(m._h, 1, cap) != 0
        msg = L.isegmi_last_error().decode()
        assert word in msg, msg
    for name, value, back, word in (("graph", 1.0, 0.0, "graph 1"), ("fp16", 1.0, 0.0, "fp16"), ("arch_c4", 1.0, 0.0, "arch_c4"), ("mask_on", 1.0, 0.0, "mask_on 1"),
                                    ("keypoint_on", 1.0, 0.0, "keypoint_on 1"), ("num_classes", 257.0, 81.0, "2..256"),
                                    ("rpn_fpn_post_nms_top_n", 2000.0, 300.0, "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST")):
        model.set_param(name, value)
        try:
            refused(word)
        finally:
            model.set_param(name, back)
    refused("pool_cap", 63)
    refused("pool_cap", 8193)
    assert L.isegmi_maskrcnn_aug_merge(model._h) != 0 and b"aug_begin" in L.isegmi_last_error()
    x, hw = fc.tiny_batch()
    r = np.ones((1, 2), np.float32)
    assert L.isegmi_maskrcnn_aug_view(model._h, model.input_buffer(0).ptr, np.ascontiguousarray(hw, np.int32).ctypes.data, 1, 128, 160, 0, r.ctypes.data) != 0
    assert b"aug_begin" in L.isegmi_last_error()
    assert L.isegmi_maskrcnn_aug_begin(model._h, 1, 64) == 0    # what is built is accepted
    out = model.detect_aug(images()[:1], configs()[1])          # and a sequence left open is simply begun again
    assert len(out[0]) > 0


def _expected_rows(model, batches, ids):
    """detect_aug per batch, resized to the original sizes, as COCO rows"""
    from isegmi.coco import maskrcnn_results
    mc, aug = configs()
    rows = {}
    for b in batches:
        out = model.detect_aug([images()[i] for i in b], aug, MIN_SIZE, MAX_SIZE)
        for i, p in zip(b, out):
            h, w = images()[i].shape[:2]
            p = p.resize((w, h))
            rows[i] = maskrcnn_results(ids[i], p.bbox, p.get_field("scores"), p.get_field("labels"))
    return [r for i in sorted(rows) for r in rows[i]]


def test_cocodemo_and_inference_use_detect_aug(ffi):
    from isegmi.predictor import COCODemo, inference
    demo = COCODemo(node(), min_image_size=MIN_SIZE, confidence_threshold=0.0, state_dict=state_dict(), max_image_size=MAX_SIZE, max_batch=2)
    try:
        m = demo.engine()
        assert demo.bbox_aug == configs()[1] and demo.box_only and (m.H, m.W) == (224, 224)
        ids = [10, 11, 12]
        single = _expected_rows(m, [[0], [1], [2]], ids)
        from isegmi.coco import maskrcnn_results
        direct = []
        for i, im in enumerate(images()):
            p = demo.compute_prediction(im)
            assert not p.has_field("mask") and p.size == (im.shape[1], im.shape[0])
            direct += maskrcnn_results(ids[i], p.bbox, p.get_field("scores"), p.get_field("labels"))
        assert direct == single and len(direct) > 50
        st = {}
        res = inference(demo, images(), image_ids=ids, batch_size=2, stats=st)     # images 0 and 2 share every view's canvas: one batch of two
        assert st["steps"] == 2 and st["images"] == 3
        assert res == _expected_rows(m, [[0, 2], [1]], ids)
        assert inference(demo, images(), image_ids=ids, batch_size=1, workers=0) == single
        out = demo.run_on_opencv_image(images()[0])
        assert out.shape == images()[0].shape and (out != images()[0]).any()
        with pytest.raises(ValueError, match=r"world=2.*TEST\.BBOX_AUG"):
            inference(demo, images(), world=2)
        small = COCODemo(node(), min_image_size=MIN_SIZE, confidence_threshold=0.0, state_dict=state_dict(), max_image_size=MAX_SIZE, max_batch=1, aug_canvas=(160, 160))
        try:
            with pytest.raises(ValueError, match=r"canvas 128x192.*160x160"):   # the 128-scale view of a 150 x 200 image (128 x 170) does not fit
                small.compute_prediction(images()[0])
            eng = small.engine()
            assert eng._canvas == (160, 160) and (eng._hw == 160).all()   # the refusal left the wrapper as reserve() had it: nothing was enqueued
        finally:
            small.close()
    finally:
        demo.close()


def test_cli_test_net_writes_the_same_rows(ffi, tmp_path):
    from PIL import Image
    from isegmi import cli
    from isegmi.predictor import COCODemo, inference
    src = tmp_path / "in"
    src.mkdir()
    for i, im in enumerate(images()[:2]):
        Image.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(src / ("im%d.png" % i))
    yaml = os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml")
    opts = ["MODEL.WEIGHT", "random"] + [str(v) for v in OVERRIDES]
    out = cli.main(["test_net", "--config-file", yaml, "--images", str(src), "--output", str(tmp_path / "a.json")] + opts)
    back = json.load(open(tmp_path / "a.json"))
    assert len(back) == len(out) > 50 and all(set(r) == {"image_id", "category_id", "bbox", "score"} for r in back)
    files = sorted(os.listdir(src))
    loaded = [cli._load_image_bgr(str(src / f)) for f in files]
    assert all(np.array_equal(a, b) for a, b in zip(loaded, images()[:2]))
    c = node()
    c.MODEL.WEIGHT = "random"
    demo = COCODemo(c, min_image_size=MIN_SIZE, confidence_threshold=0.0, max_image_size=MAX_SIZE, max_batch=2)
    try:
        assert json.loads(json.dumps(inference(demo, loaded, batch_size=2))) == back
    finally:
        demo.close()
