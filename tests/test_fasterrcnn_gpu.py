"""Faster R-CNN on the HIP engine (MODEL.MASK_ON False): the box-only forward against the oracle and against the mask engine built beside
it on the same weights, mask_on toggled on a live engine, the class count and the class-agnostic regression stage by stage on the engine's own
intermediates, the box-only record block through COCODemo / inference(), and the refusals.  Every comparison is bit for bit."""
import dataclasses
import os

import numpy as np
import pytest

import fasterrcnn_cases as fc
from oracle import ora

pytestmark = pytest.mark.gpu

SEED_CLASSES = 5   # the seed whose weights give several labels at 9 classes on the 128 x 160 canvas (asserted below from the reference side)


def _box_cfg(**kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return dataclasses.replace(MaskRCNNConfig(), MASK_ON=False, **kw)


def _forward(model, x, hw):
    n = x.shape[0]
    model.upload(x, hw); model.forward_device(n); model.sync()
    return fc.fetch_dets(model, n)


def test_fpn_fp32_box_only_equals_the_oracle_and_the_mask_engine(ffi):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw, ref, rd = fc.small_reference()
    box = MaskRCNN(maskrcnn_state_dict(1234, mask=False), x.shape[1], x.shape[2], cfg=_box_cfg(), max_batch=2)
    mask = MaskRCNN(fc.full_state_dict(), x.shape[1], x.shape[2], max_batch=2)
    try:
        assert box.box_only and not mask.box_only
        mem_box, mem_mask = box.reserve(), mask.reserve()
        assert mem_box[1] < mem_mask[1] and mem_box[0] < mem_mask[0]          # fewer activation bytes, and no mask-head weights
        out = box(x, hw)
        for name in ("P2", "P3", "P4", "P5", "P6"):
            assert np.array_equal(box.fetch(name, 2), ref.feats[name]), name
        pc = box.fetch("proposal_count", 2); pr = box.fetch("proposals", 2); ps = box.fetch("proposal_scores", 2)
        total = 0
        for n in range(2):
            r = rd[n]
            assert pc[n] == len(r["proposals"])
            assert np.array_equal(ps[n, : pc[n]], r["proposal_scores"]) and np.array_equal(pr[n, : pc[n]], r["proposals"])
            bl = out[n]
            assert not bl.has_field("mask") and sorted(bl.fields()) == ["labels", "scores"]
            assert len(bl) == len(r["score"]) and np.array_equal(bl.get_field("labels"), r["label"].astype(np.int64))
            assert np.array_equal(bl.get_field("scores"), r["score"]) and np.array_equal(bl.bbox, r["box"])
            total += len(bl)
        assert total > 20
        for name in ("det.mask28", "mask.roi_feat", "mask.deconv", "mask.roi_table", "det.masks"):   # never allocated, reserve() included
            with pytest.raises(ffi.IsegmiError, match="no such buffer"):
                box.fetch(name)
        assert mask.fetch("det.mask28", 2).shape == (2, 100, 28, 28)
        got_box = fc.fetch_dets(box, 2)
        got_mask = _forward(mask, x, hw)
        fc.assert_same_dets(got_box, got_mask, "box-only vs mask engine")
        assert fc.count_launches(box, 2) < fc.count_launches(mask, 2)
        fc.assert_same_dets(fc.fetch_dets(box, 2), got_box, "after the counting passes")
    finally:
        box.close(); mask.close()


def _same_weights_equality(full_sd, box_sd, cfg, x, hw, **kw):
    from isegmi.maskrcnn import MaskRCNN
    box = MaskRCNN(box_sd, x.shape[1], x.shape[2], cfg=dataclasses.replace(cfg, MASK_ON=False), max_batch=x.shape[0], **kw)
    mask = MaskRCNN(full_sd, x.shape[1], x.shape[2], cfg=cfg, max_batch=x.shape[0], **kw)
    try:
        a, b = _forward(box, x, hw), _forward(mask, x, hw)
        fc.assert_same_dets(a, b)
        assert int(a["det.count"].sum()) > 10
        with pytest.raises(Exception, match="no such buffer"):
            box.fetch(box.mask_buf)
        assert mask.fetch(mask.mask_buf, x.shape[0]).shape[0] == x.shape[0]
        return a
    finally:
        box.close(); mask.close()


def test_fp16_box_only_equals_the_mask_engine(ffi):
    from isegmi.maskrcnn import MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.small_reference()[:2]
    _same_weights_equality(fc.full_state_dict(), maskrcnn_state_dict(1234, mask=False), MaskRCNNConfig(), x, hw, fp16=True)


def test_groupnorm_box_only_equals_the_mask_engine(ffi):
    import maskrcnn_gn_common as gc
    from isegmi.maskrcnn import prepare_images
    from isegmi.weights import maskrcnn_state_dict
    x, hw = prepare_images(gc.small_images())
    _same_weights_equality(gc.state_dict(), maskrcnn_state_dict(gc.SEED, gn=True, mask=False), gc.gn_cfg(), x, hw)


def test_c4_box_only_equals_the_mask_engine_and_the_oracle(ffi):
    """R-50-C4 on one ~200 x 260 image with RPN post-NMS top-n 100: the res5 head runs on 100 RoIs, and box-only skips its second pass."""
    from isegmi.maskrcnn import MaskRCNNConfig, prepare_images
    from isegmi.weights import maskrcnn_c4_state_dict
    from oracle.maskrcnn_ref import MaskRCNNRef
    x, hw = prepare_images([np.random.default_rng(5).uniform(0, 255, (200, 260, 3)).astype(np.float32)], 16)
    cfg = dataclasses.replace(MaskRCNNConfig.c4(), RPN_POST_NMS_TOP_N_TEST=100)
    full = maskrcnn_c4_state_dict(1234)
    got = _same_weights_equality(full, maskrcnn_c4_state_dict(1234, mask=False), cfg, x, hw)
    r = MaskRCNNRef(full).forward_c4(x, hw, pre_nms=6000, post_nms=100)[0]
    assert got["det.count"][0] == len(r["score"]) > 10
    assert np.array_equal(got["det.label"][0], r["label"]) and np.array_equal(got["det.score"][0], r["score"]) and np.array_equal(got["det.box"][0], r["box"])


def test_mask_on_toggled_on_a_live_mask_engine(ffi):
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = fc.small_reference()
    m = MaskRCNN(fc.full_state_dict(), x.shape[1], x.shape[2], max_batch=2)
    try:
        def full_result():
            out = m(x, hw)
            m.paste_device(256, 352); m.sync()
            return out, m.fetch("det.masks", 2).copy()
        first, planes1 = full_result()
        m.set_mask_on(False)
        assert m.box_only
        second = m(x, hw)
        with pytest.raises(RuntimeError, match="paste_device"):
            m.paste_device(256, 352)
        m.set_mask_on(True)
        third, planes3 = full_result()
        for n in range(2):
            a, b, c = first[n], second[n], third[n]
            assert a.has_field("mask") and c.has_field("mask") and not b.has_field("mask")
            for u in (b, c):
                assert np.array_equal(a.bbox, u.bbox) and np.array_equal(a.get_field("scores"), u.get_field("scores"))
                assert np.array_equal(a.get_field("labels"), u.get_field("labels"))
            assert np.array_equal(a.get_field("mask"), c.get_field("mask")) and a.get_field("mask").any()
            r = rd[n]   # the second result is test 1's: the oracle's boxes, scores and labels
            assert np.array_equal(b.bbox, r["box"]) and np.array_equal(b.get_field("scores"), r["score"]) and np.array_equal(b.get_field("labels"), r["label"].astype(np.int64))
            assert np.array_equal(a.get_field("mask")[:, 0], r["mask28"])
        assert np.array_equal(planes1, planes3) and planes1.any()
    finally:
        m.close()


@pytest.mark.parametrize("ncls", [2, 9, 257])
def test_class_count_stage_by_stage(ffi, ncls):
    """NUM_CLASSES 2, 9 and 257, box-only, 128 x 160: the predictor layer from the engine's own fc7 rows, the detections from the engine's own predictor
    rows and proposals."""
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.tiny_batch()
    sd = maskrcnn_state_dict(SEED_CLASSES, mask=False, num_classes=ncls)
    m = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=_box_cfg(NUM_CLASSES=ncls), max_batch=1)
    try:
        got = _forward(m, x, hw)
        f7, cb, props, w, b = fc.predictor_rows(m, sd)
        assert cb.shape[1] == 5 * ncls and len(props) > 100
        assert np.array_equal(ora.conv2d(f7, w, 1, 0, None, b, None, 0).reshape(cb.shape), cb)
        rb, rs, rl = ora.box_postprocess(cb[:, :ncls], cb[:, ncls:], props, float(hw[0][1]), float(hw[0][0]), 0.05, 0.5, 100, 0, 100)
        assert got["det.count"][0] == len(rs) > 0
        assert np.array_equal(got["det.label"][0], rl) and np.array_equal(got["det.score"][0], rs) and np.array_equal(got["det.box"][0], rb)
        assert rl.min() >= 1 and rl.max() <= ncls - 1
        if ncls == 9:
            assert len(set(rl.tolist())) >= 2
    finally:
        m.close()


def test_mask_model_at_nine_classes_selects_the_labels_channel(ffi):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.tiny_batch()
    sd = maskrcnn_state_dict(SEED_CLASSES, num_classes=9)
    m = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=dataclasses.replace(MaskRCNNConfig(), NUM_CLASSES=9), max_batch=1)
    try:
        got = _forward(m, x, hw)
        D = int(got["det.count"][0])
        labels = got["det.label"][0]
        assert D > 0 and len(set(labels.tolist())) >= 2
        f7, cb, props, w, b = fc.predictor_rows(m, sd)
        rb, rs, rl = ora.box_postprocess(cb[:, :9], cb[:, 9:], props, float(hw[0][1]), float(hw[0][0]), 0.05, 0.5, 100, 0, 100)
        assert np.array_equal(labels, rl) and np.array_equal(got["det.box"][0], rb)
        up = m.fetch("mask.deconv")[:D]
        want = ora.mask_logits_select(up.reshape(D, 784, 256), sd["roi_heads.mask.predictor.mask_fcn_logits.weight"].reshape(9, 256),
                                      sd["roi_heads.mask.predictor.mask_fcn_logits.bias"], rl)
        assert np.array_equal(m.fetch("det.mask28", 1)[0, :D].reshape(D, 784), want)
    finally:
        m.close()


def test_class_agnostic_engine_from_its_fetched_rows(ffi):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.tiny_batch()
    sd = maskrcnn_state_dict(SEED_CLASSES, mask=False, num_classes=9, cls_agnostic=True)
    m = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=_box_cfg(NUM_CLASSES=9, CLS_AGNOSTIC_BBOX_REG=True), max_batch=1)
    try:
        got = _forward(m, x, hw)
        f7, cb, props, w, b = fc.predictor_rows(m, sd)
        assert cb.shape[1] == 9 + 8
        assert np.array_equal(ora.conv2d(f7, w, 1, 0, None, b, None, 0).reshape(cb.shape), cb)
        rb, rs, rl = ora.box_postprocess(cb[:, :9], fc.agnostic_regr(cb[:, 9:], 9), props, float(hw[0][1]), float(hw[0][0]), 0.05, 0.5, 100, 0, 100)
        assert got["det.count"][0] == len(rs) > 0 and len(set(rl.tolist())) >= 2
        assert np.array_equal(got["det.label"][0], rl) and np.array_equal(got["det.score"][0], rs) and np.array_equal(got["det.box"][0], rb)
        pb, _, _ = ora.box_postprocess(cb[:, :9], fc.per_class_reading(cb[:, 9:], 9), props, float(hw[0][1]), float(hw[0][0]), 0.05, 0.5, 100, 0, 100)
        assert not (pb.shape == rb.shape and np.array_equal(pb, rb))            # the other reading is another answer here too
    finally:
        m.close()


def _demo_images():
    from conftest import smooth_field
    rng = np.random.default_rng(41)
    return [rng.integers(0, 256, (150, 200, 3)).astype(np.uint8), np.ascontiguousarray(smooth_field(7, 200, 150), np.uint8),
            rng.integers(0, 256, (150, 200, 3)).astype(np.uint8)]


def test_cocodemo_and_inference_write_bbox_results(ffi, tmp_path):
    """COCODemo with the faster_rcnn yaml on three small images (two canvases, bs = 2): inference() -- the box-only record block through the two-slot
    download, and again through the RCCL all-gather of a world of one, and from a lazy source -- equals the per-image compute_prediction results."""
    import json
    from conftest import ROOT
    from isegmi.coco import maskrcnn_results
    from isegmi.config import cfg
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.predictor import COCODemo, inference
    from isegmi.weights import maskrcnn_state_dict
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x.yaml"))
    images = _demo_images()
    shapes = [im.shape[:2] for im in images]
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, state_dict=maskrcnn_state_dict(1234, mask=False), max_image_size=320, max_batch=2)
    try:
        model = demo.engine()
        assert demo.box_only and isinstance(model, MaskRCNN) and model.box_only
        assert model.coco_record_bytes(2) == (fc.box_block_bytes(2, 100), fc.box_block_bytes(2, 100))
        assert model.coco_record_bytes(1)[0] == fc.box_block_bytes(1, 100)
        direct = []
        for i, im in enumerate(images):
            p = demo.compute_prediction(im)
            assert not p.has_field("mask") and p.size == (im.shape[1], im.shape[0])
            direct += maskrcnn_results(10 + i, p.bbox, p.get_field("scores"), p.get_field("labels"))
        assert len(direct) > 20
        st = {}
        res = inference(demo, images, image_ids=[10, 11, 12], batch_size=2, stats=st)
        assert st["steps"] == 2 and st["images"] == 3
        gathered = inference(demo, images, image_ids=[10, 11, 12], batch_size=2, force_gather=True)
        lazy = inference(demo, lambda i: images[i], image_ids=[10, 11, 12], batch_size=1, sizes=shapes, workers=0)
        path = tmp_path / "bbox.json"
        path.write_text(json.dumps(res))
        back = json.loads(path.read_text())
        assert all("segmentation" not in d and len(d["bbox"]) == 4 for d in back)
        assert res == direct and gathered == direct and lazy == direct
        out = demo.run_on_opencv_image(images[0])
        assert out.shape == images[0].shape and out.dtype == np.uint8 and (out != images[0]).any()
    finally:
        demo.close()


def test_zero_detections_give_empty_results_and_a_zero_count_section(ffi):
    from isegmi.dist import coco_record_layout
    from isegmi.pipeline import RecordPipeline
    from isegmi.predictor import COCODemo, inference
    from isegmi.weights import maskrcnn_state_dict
    sd = maskrcnn_state_dict(1234, mask=False)
    sd["roi_heads.box.predictor.cls_score.bias"] = sd["roi_heads.box.predictor.cls_score.bias"].copy()
    sd["roi_heads.box.predictor.cls_score.bias"][0] += 50.0
    images = _demo_images()
    demo = COCODemo(_box_cfg(), min_image_size=192, confidence_threshold=0.0, state_dict=sd, max_image_size=320, max_batch=2)
    try:
        assert inference(demo, images, batch_size=2) == []
        model = demo.engine()
        # the block itself: one image in a block of two slots
        from isegmi.transforms import maskrcnn_resize_u8
        n = model.upload_u8([maskrcnn_resize_u8(images[0], 192, 320)])
        model.forward_device(n)
        model.set_output_sizes([(200, 150)])
        with RecordPipeline(model, 2) as pipe:
            assert pipe.box_only and pipe.nbytes == fc.box_block_bytes(2, 100) == coco_record_layout(2, 100, 2, False, 0, box_only=True)[2]
            pipe.submit("step")
            (meta, (rec,)), = pipe.flush()
            assert meta == "step" and not rec["count"].any() and not rec["status"].any() and rec["overflow"] is None
            raw = pipe.pin[0].array.copy()
        off, nb = coco_record_layout(2, 100, 2, False, 0, box_only=True)[0]["count"][:2]
        assert not raw[off:off + nb].any() and not raw[:16].any()
    finally:
        demo.close()


def test_box_records_scale_the_boxes_and_zero_the_empty_slot(ffi):
    """isegmi_engine_pack_box_records on its own: one image in a block of two slots, boxes = det.box * ratio in fp32, the second slot zero."""
    from isegmi.dist import unpack_coco_records
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.tiny_batch()
    m = MaskRCNN(maskrcnn_state_dict(SEED_CLASSES, mask=False), x.shape[1], x.shape[2], cfg=_box_cfg(), max_batch=2)
    try:
        got = _forward(m, x, hw)
        D = int(got["det.count"][0])
        assert D > 0
        m.set_output_sizes([(333, 517)])
        dev = ffi.DeviceBuffer.from_numpy(np.full(fc.box_block_bytes(2, 100) + 64, 0xa5, np.uint8))   # dirty: everything inside the block is written
        assert m.pack_box_records(dev, 2) == fc.box_block_bytes(2, 100)
        m.sync()
        raw = dev.numpy()
        assert (raw[fc.box_block_bytes(2, 100):] == 0xa5).all()                                        # and nothing past it
        rec = unpack_coco_records(raw, 2, 100, 2, box_only=True)
        ratio = np.array([333 / hw[0][1], 517 / hw[0][0]] * 2).astype(np.float32)
        assert rec["count"].tolist() == [D, 0] and not rec["status"].any()
        assert np.array_equal(rec["box"][0, :D], got["det.box"][0] * ratio) and np.array_equal(rec["score"][0, :D], got["det.score"][0])
        assert np.array_equal(rec["label"][0, :D], got["det.label"][0])
        assert not rec["box"][0, D:].any() and not rec["box"][1].any() and not rec["score"][1].any() and not rec["label"][1].any()
        small = ffi.DeviceBuffer((fc.box_block_bytes(2, 100) - 8,), np.uint8)
        with pytest.raises(ffi.IsegmiError, match="too small"):
            m.pack_box_records(small, 2)
    finally:
        m.close()


def test_refusals(ffi):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    x, hw = fc.tiny_batch()
    box_sd = maskrcnn_state_dict(SEED_CLASSES, mask=False)
    with pytest.raises(ValueError, match=r"MODEL\.MASK_ON"):                      # MASK_ON True with a mask-less dict
        MaskRCNN(box_sd, x.shape[1], x.shape[2], cfg=MaskRCNNConfig(), max_batch=1)
    nine = dict(box_sd)                                                           # nine logits, but 324 deltas: neither 4 * 9 nor 2 * 4
    for k in ("weight", "bias"):
        nine["roi_heads.box.predictor.cls_score." + k] = box_sd["roi_heads.box.predictor.cls_score." + k][:9]
    with pytest.raises(ValueError, match=r"bbox_pred has 324 outputs: 9 classes need 36 = 4 \* NUM_CLASSES"):
        MaskRCNN(nine, x.shape[1], x.shape[2], cfg=_box_cfg(NUM_CLASSES=9), max_batch=1)
    with pytest.raises(ValueError, match=r"need 8 = 2 \* 4"):
        MaskRCNN(nine, x.shape[1], x.shape[2], cfg=_box_cfg(NUM_CLASSES=9, CLS_AGNOSTIC_BBOX_REG=True), max_batch=1)
    m = MaskRCNN(maskrcnn_state_dict(SEED_CLASSES), x.shape[1], x.shape[2], cfg=_box_cfg(), max_batch=1)   # present mask keys are ignored
    try:
        got = _forward(m, x, hw)
        assert got["det.count"][0] > 0
        with pytest.raises(RuntimeError, match="paste_device"):
            m.paste_device(128, 160)
        with pytest.raises(RuntimeError, match="rle_device"):
            m.rle_device()
        with pytest.raises(ValueError, match="set_mask_on"):                       # its mask weights were never loaded
            m.set_mask_on(True)
        import ctypes as C
        r = np.ones((1, 2), np.float32)
        assert ffi.lib().isegmi_maskrcnn_paste(m._h, r.ctypes.data_as(C.c_void_p), 128, 160) != 0   # the C entry points refuse by name too
        assert b"box-only" in ffi.lib().isegmi_last_error()
        assert ffi.lib().isegmi_engine_rle(m._h, None) != 0 and b"box-only" in ffi.lib().isegmi_last_error()
        # a cls_bbox width that fits neither form, in the engine: 81 classes need 81+324, or 81+8 when class-agnostic
        w = np.zeros((81 + 12, 1, 1, 1024), np.float32)
        m._set_conv_krsc("roi_heads.box.predictor.cls_bbox", w, None, np.zeros(81 + 12, np.float32))
        with pytest.raises(ffi.IsegmiError, match=r"93 outputs; 81 classes need 81\+324 \(per-class"):
            m.forward_device(1)
        m.sync()
        m.set_param("cls_agnostic", 1.0)
        with pytest.raises(ffi.IsegmiError, match=r"81\+8 \(class-agnostic"):
            m.forward_device(1)
        m.sync()
    finally:
        m.close()
