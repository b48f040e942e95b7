"""The resize on the device through the engines: upload_original_u8 against upload_u8(maskrcnn_resize_u8(...)), the asynchronous path with its
upload pending, detect / aug_enqueue / YoloDetector.detect / inference() in the two modes, and host-mode steps around a device-mode step.  Small engines
(MIN_SIZE_TEST 96 / MAX_SIZE_TEST 160 box-only, 192 / 320 with masks, a 64 x 96 YOLOv3 canvas); every comparison is bit for bit."""
import functools
import json
import os

import numpy as np
import pytest

import fasterrcnn_cases as fc
import yolov3_cases as yc
from conftest import ROOT, smooth_field

pytestmark = pytest.mark.gpu
MIN_SIZE, MAX_SIZE = 96, 160
OVERRIDES = ["INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE, "TEST.BBOX_AUG.SCALES", (64, 128), "TEST.BBOX_AUG.MAX_SIZE", 224,
             "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 300, "MODEL.ROI_HEADS.SCORE_THRESH", 0.04]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def images():
    """a landscape and a portrait that are scaled up, one that is scaled down, one already at MIN_SIZE (get_size returns its own size)"""
    out = [np.ascontiguousarray(smooth_field(3, 75, 100), np.uint8), np.ascontiguousarray(smooth_field(7, 105, 75), np.uint8),
           np.random.default_rng(5).integers(0, 256, (301, 403, 3), dtype=np.uint8), np.ascontiguousarray(smooth_field(11, 96, 128), np.uint8)]
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
def box_state_dict():
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(1234, mask=False)


@pytest.fixture(scope="module")
def model(ffi):
    """the box-only engine of the bbox-aug tests: canvases up to 224 x 224, two images"""
    from isegmi.maskrcnn import MaskRCNN, bbox_aug_engine_side
    mc, aug = configs()
    side = bbox_aug_engine_side(mc, aug)
    m = MaskRCNN(box_state_dict(), side, side, cfg=mc, max_batch=2)
    yield m
    m.close()


def input_after(model, upload, slot=0):
    """The canvas batch in input buffer `slot` after upload(): the buffer is poisoned first, so a canvas element the front end leaves alone is a NaN."""
    model.sync()
    model.input_buffer(slot).poison()
    n = upload()
    model.sync()
    H, W = model._canvas
    flat = model.input_buffer(slot).numpy().reshape(-1)[:(n or len(model._hw)) * H * W * 3]
    assert not np.isnan(flat).any()
    return bits(flat), model._canvas, model._hw.copy()


@pytest.mark.parametrize("which", [(0, 1), (1,), (2,), (3,), (2, 3), (3, 0)], ids=["mixed", "upscale", "downscale", "at-size", "down+at-size", "at-size+up"])
def test_input_buffer_equals_the_host_path(model, which):
    from isegmi.transforms import maskrcnn_resize_u8
    ims = [images()[i] for i in which]
    resized = [maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in ims]
    if which == (3,):
        assert resized[0].shape == ims[0].shape
    want, canvas, hw = input_after(model, lambda: model.upload_u8(resized))
    got, canvas2, hw2 = input_after(model, lambda: model.upload_original_u8(ims, 0, MIN_SIZE, MAX_SIZE))
    assert canvas == canvas2 and np.array_equal(hw, hw2)
    assert np.array_equal(got, want), int((got != want).sum())


def test_async_path_with_the_upload_pending(ffi, model):
    """plan.write into pinned memory, upload_async and the resize launch enqueued back to back on the copy stream: nothing waits in between"""
    from isegmi.transforms import maskrcnn_resize_u8
    ims = [images()[2], images()[3]]
    want, canvas, hw = input_after(model, lambda: model.upload_u8([maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in ims], slot=1), slot=1)
    plan, phw = model.original_plan([im.shape[:2] for im in ims], MIN_SIZE, MAX_SIZE)
    pin = ffi.PinnedBuffer((plan.nbytes,), np.uint8)
    try:
        assert plan.write(pin.array, ims) == plan.nbytes

        def up():
            model.upload_original_u8_async(pin, plan, phw, slot=1)
            return len(ims)
        got, canvas2, hw2 = input_after(model, up, slot=1)
        assert canvas == canvas2 and np.array_equal(hw, hw2) and np.array_equal(got, want)
        # and a forward enqueued right behind it, the upload still pending, reads what the host path's forward reads
        model.upload_u8([maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in ims])
        model.forward_device(2); model.sync()
        ref = fc.fetch_dets(model, 2)
        model.upload_original_u8_async(pin, plan, phw, slot=1)
        model.forward_device(2, slot=1); model.sync()
        fc.assert_same_dets(fc.fetch_dets(model, 2), ref, "forward behind a pending upload")
        assert int(ref["det.count"].sum()) > 0   # (the noise image detects nothing under these weights, the smooth one does)
    finally:
        model.sync()
        pin.free()


def test_detect_and_host_steps_around_a_device_step(model):
    from isegmi.transforms import maskrcnn_resize_u8
    ims = [images()[0], images()[1]]
    resized = [maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in ims]

    def rows(out):
        return [(bits(p.bbox), bits(p.get_field("scores")), p.get_field("labels"), p.size) for p in out]
    before = rows(model(resized))
    dev = rows(model.detect_original(ims, MIN_SIZE, MAX_SIZE))
    after = rows(model(resized))
    assert sum(len(r[2]) for r in before) > 0
    for a, b, c in zip(before, dev, after):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)


def test_aug_enqueue_is_identical_in_the_two_modes(model):
    """two scales and every mirror image: six views of two images of different sizes from ONE upload of the two originals"""
    mc, aug = configs()
    assert aug.H_FLIP and aug.SCALE_H_FLIP and len(aug.SCALES) == 2
    ims = [images()[0], images()[1]]
    host = model.detect_aug(ims, aug, MIN_SIZE, MAX_SIZE)
    want, want_total = fc.fetch_dets(model, 2), model.fetch("aug.pool_total", 2)
    dev = model.detect_aug(ims, aug, MIN_SIZE, MAX_SIZE, resize="device")
    fc.assert_same_dets(fc.fetch_dets(model, 2), want, "six views")
    assert np.array_equal(model.fetch("aug.pool_total", 2), want_total) and int(want["det.count"].min()) > 0
    assert [p.size for p in dev] == [p.size for p in host]
    with pytest.raises(ValueError, match="resize"):
        model.aug_enqueue(ims, aug, resize="gpu")
    again = model.detect_aug(ims, aug, MIN_SIZE, MAX_SIZE)   # the host mode behind a device-mode pass
    fc.assert_same_dets(fc.fetch_dets(model, 2), want, "host mode again")
    assert len(again) == 2


def test_yolo_detector_is_identical_in_the_two_modes(ffi):
    """a 64 x 96 canvas, a portrait and a landscape image (padding left / right and top / bottom), and one already at the letterbox size"""
    from isegmi.transforms import yolo_letterbox
    from isegmi.yolov3 import YoloDetector, YoloV3Config
    rng = np.random.default_rng(3)
    ims = [rng.integers(0, 256, (90, 50, 3), dtype=np.uint8), rng.integers(0, 256, (40, 170, 3), dtype=np.uint8), rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)]
    cfg = YoloV3Config(height=64, width=96, conf_thresh=yc.ENGINE_CONF)
    host, dev = YoloDetector(yc.engine_weights(), cfg, max_batch=3), None
    try:
        dev = YoloDetector(yc.engine_weights(), cfg, max_batch=3, resize="device")
        net = dev.net
        net.input_buffer(0).poison()
        n, geos = net.upload_original_u8(ims)
        net.sync()
        lb = [yolo_letterbox(im, 64, 96) for im in ims]
        assert [g for _, g in lb] == geos
        assert np.array_equal(bits(net.input_buffer(0).numpy()[:n]), bits(np.stack([x for x, _ in lb])))
        a, b = host.detect(ims), dev.detect(ims)
        assert sum(len(s) for _, s, _ in a) > 0
        for (ba, sa, la), (bb, sb, lb_) in zip(a, b):
            assert np.array_equal(bits(ba), bits(bb)) and np.array_equal(bits(sa), bits(sb)) and np.array_equal(la, lb_)
    finally:
        host.close()
        if dev is not None:
            dev.close()


def test_inference_box_only_and_bbox_aug_in_the_two_modes(ffi):
    from isegmi.predictor import COCODemo, inference
    mc, aug = configs()
    ims = list(images())
    for kw in (dict(), dict(bbox_aug=aug)):
        demo = COCODemo(mc, min_image_size=MIN_SIZE, confidence_threshold=0.0, state_dict=box_state_dict(), max_image_size=MAX_SIZE, max_batch=2, **kw)
        try:
            want = inference(demo, ims, image_ids=[10, 11, 12, 13], batch_size=2)
            st = {}
            got = inference(demo, ims, image_ids=[10, 11, 12, 13], batch_size=2, resize="device", stats=st)
            assert json.dumps(got) == json.dumps(want) and len(want) > 0 and st["images"] == 4
            assert json.dumps(inference(demo, lambda i: ims[i], image_ids=[10, 11, 12, 13], batch_size=1, workers=0, resize="device",
                                        sizes=[im.shape[:2] for im in ims])) == json.dumps(inference(demo, ims, image_ids=[10, 11, 12, 13], batch_size=1))
            demo.resize = "device"   # COCODemo(cfg, resize="device"): compute_prediction and inference() take the predictor's mode
            ps = [demo.compute_prediction(im) for im in ims]
            demo.resize = "host"
            qs = [demo.compute_prediction(im) for im in ims]
            assert sum(len(q) for q in qs) > 0   # (the noise image alone detects nothing under these weights: the guard is over all four)
            for p, q in zip(ps, qs):
                assert np.array_equal(bits(p.bbox), bits(q.bbox)) and np.array_equal(bits(p.get_field("scores")), bits(q.get_field("scores")))
                assert np.array_equal(p.get_field("labels"), q.get_field("labels")) and p.size == q.size
        finally:
            demo.close()


def test_inference_with_masks_in_the_two_modes(ffi):
    from isegmi.predictor import COCODemo, inference
    from isegmi.weights import maskrcnn_state_dict
    ims = [np.ascontiguousarray(smooth_field(100 + i, h, w), np.uint8) for i, (h, w) in enumerate(((150, 200), (200, 150), (150, 200), (400, 610)))]
    demo = COCODemo(None, min_image_size=192, confidence_threshold=0.0, state_dict=maskrcnn_state_dict(1234), max_image_size=320, max_batch=2, resize="device")
    try:
        got = inference(demo, ims, batch_size=2)                      # the predictor's own mode
        want = inference(demo, ims, batch_size=2, resize="host")
        assert json.dumps(got) == json.dumps(want) and len(want) > 0 and all("segmentation" in r for r in want)
        p = demo.compute_prediction(ims[3])
        demo.resize = "host"
        q = demo.compute_prediction(ims[3])
        assert np.array_equal(bits(p.bbox), bits(q.bbox)) and np.array_equal(p.get_field("mask"), q.get_field("mask"))
    finally:
        demo.close()
