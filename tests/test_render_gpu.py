"""The device painter behind the public entry points: COCODemo(render="device") equals render="host" bit for bit for every model family
that draws (Mask R-CNN FPN and C4, Keypoint R-CNN, Faster R-CNN, RetinaNet) without ever fetching det.masks; isegmi.yolact.render_images equals
cli._overlay of postprocess(); `eval --render=device` writes that image; isegmi_engine_paint refuses by name what it cannot draw."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -2, -3


def _image(seed, h=150, w=200):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def _yaml_cfg(name, *opts):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", name))
    c.merge_from_list(list(opts))
    return c


def _both_renders(demo, image, min_drawn=1):
    """run_on_opencv_image under render="host" and render="device" on one predictor -> (host image, device image, detections drawn, fetched names)"""
    assert demo.render == "host"
    drawn = len(demo.select_top_predictions(demo.compute_prediction(image)))
    assert drawn >= min_drawn, "the threshold of this test draws nothing: lower it"
    host = demo.run_on_opencv_image(image)
    model = demo.engine()
    fetched, fetch = [], model.fetch
    model.fetch = lambda name, rows=None: (fetched.append(name), fetch(name, rows))[1]
    before = image.copy()
    demo.render = "device"
    try:
        dev = demo.run_on_opencv_image(image)
    finally:
        demo.render = "host"
        del model.fetch
    assert np.array_equal(image, before) and dev is not image and dev.dtype == np.uint8 and dev.shape == image.shape
    assert "det.count" in fetched and "det.masks" not in fetched, fetched
    return host, dev, drawn, fetched


def _assert_same(host, dev, image):
    assert (host != image).any(), "nothing was drawn"
    if not np.array_equal(host, dev):
        bad = np.argwhere((host != dev).any(2))
        pytest.fail("%d pixels differ, first (y, x) = %s: host %s device %s" % (len(bad), bad[0].tolist(), host[tuple(bad[0])].tolist(), dev[tuple(bad[0])].tolist()))


def test_maskrcnn_device_render_equals_host(ffi):
    from isegmi.predictor import COCODemo
    from isegmi.weights import maskrcnn_state_dict
    image = _image(4)
    # (the seeded weights' best score on this image is 0.176: at 0.2 nothing would be drawn)
    demo = COCODemo(None, min_image_size=192, max_image_size=320, confidence_threshold=0.1, state_dict=maskrcnn_state_dict(1234))
    try:
        host, dev, drawn, _ = _both_renders(demo, image, min_drawn=2)
        print("mask r-cnn: %d detections drawn" % drawn)
        _assert_same(host, dev, image)
        # the engine entry point by hand: the first detection's plane alone (the planes are 150 x 200)
        model = demo.engine()
        e = np.array([[0, 0, 0, 0, 0, 0x00FF00, 0, 0]], np.int32)
        m1 = model.fetch("det.masks", 1)[0, 0]
        want = image.copy()
        want[m1 != 0] = (want[m1 != 0].astype(np.uint16) + np.array([0, 255, 0], np.uint16)) >> 1
        assert m1.any() and np.array_equal(model.paint_device(image, e), want)
        sub = np.ascontiguousarray(image[:77, :131])            # a smaller image in the planes' top-left corner
        assert np.array_equal(model.paint_device(sub, e), want[:77, :131])
        big = np.zeros((151, 200, 3), np.uint8)
        with pytest.raises(ffi.IsegmiError, match="does not fit the mask planes"):
            model.paint_device(big, e)
        with pytest.raises(ffi.IsegmiError, match="image_index"):
            model.paint_device(image, e, index=1)
        with pytest.raises(ffi.IsegmiError, match="slot outside"):
            model.paint_device(image, np.array([[model.cfg.det_cap, 0, 0, 0, 0, 0, 0, 0]], np.int32))
        with pytest.raises(ValueError):
            COCODemo(None, state_dict=demo.state_dict, render="gpu")
    finally:
        demo.close()


def test_maskrcnn_c4_yaml(ffi):
    from isegmi.predictor import COCODemo
    # the seeded C4 model scores this image at 0.046 and below: the engine's own cut goes to 0.01 and the demo draws what exceeds 0.04
    c = _yaml_cfg("e2e_mask_rcnn_R_50_C4_1x.yaml", "MODEL.ROI_HEADS.SCORE_THRESH", 0.01)
    c.MODEL.WEIGHT = "random"
    image = _image(8, 120, 180)
    demo = COCODemo(c, min_image_size=160, confidence_threshold=0.04, max_image_size=256)
    try:
        assert demo.cfg.is_c4
        host, dev, drawn, _ = _both_renders(demo, image)
        print("c4: %d detections drawn" % drawn)
        _assert_same(host, dev, image)
    finally:
        demo.close()


def test_keypointrcnn_dots(ffi):
    """confidence 0.0 draws every detection, and the seeded keypoint head's logits run into the thousands: every joint exceeds COCODemo.KP_THRESH"""
    from isegmi.predictor import COCODemo
    from isegmi.render import keypoint_dots
    from isegmi.weights import keypointrcnn_state_dict
    c = _yaml_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "MODEL.ROI_HEADS.SCORE_THRESH", 0.012)
    image = _image(41)
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, state_dict=keypointrcnn_state_dict(1234), max_image_size=320)
    try:
        pred = demo.select_top_predictions(demo.compute_prediction(image))
        dots = keypoint_dots(pred, demo.KP_THRESH)
        print("keypoint r-cnn: %d detections, %d dots, logits up to %.3f" % (len(pred), len(dots), float(pred.get_field("keypoint_logits").max())))
        assert len(dots) >= 1, "no keypoint logit above the threshold: no dot is drawn"
        host, dev, _, fetched = _both_renders(demo, image)
        assert "det.kpt" in fetched
        _assert_same(host, dev, image)
        boxes_only = demo.overlay_class_names(_paint_boxes(demo, image, pred), pred)
        assert (host != boxes_only).any(), "the dots changed nothing"
    finally:
        demo.close()


def _paint_boxes(demo, image, pred):
    from isegmi.render import demo_entries
    return demo.engine().paint_device(image, demo_entries(pred, image.shape[0], image.shape[1], with_masks=False))


@pytest.mark.parametrize("family", ["faster", "retinanet"])
def test_box_only_models_draw_slotless_entries(ffi, family):
    from isegmi.predictor import COCODemo
    from isegmi.render import demo_entries
    if family == "faster":
        from isegmi.weights import maskrcnn_state_dict
        c, sd, thr = _yaml_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml"), maskrcnn_state_dict(1234, mask=False), 0.1
    else:
        import retinanet_common as rc
        c, sd, thr = _yaml_cfg("retinanet_R-50-FPN_1x.yaml"), rc.state_dict(), 0.05
    image = _image(41)
    demo = COCODemo(c, min_image_size=192, confidence_threshold=thr, state_dict=sd, max_image_size=320)
    try:
        host, dev, drawn, _ = _both_renders(demo, image)
        print("%s: %d detections drawn" % (family, drawn))
        _assert_same(host, dev, image)
        pred = demo.select_top_predictions(demo.compute_prediction(image))
        e = demo_entries(pred, 150, 200, with_masks=False)
        assert len(e) == drawn and (e[:, 0] == -1).all()
        # a slot on an engine without masks: refused by name, nothing drawn
        model = demo.engine()
        e[0, 0] = 0
        with pytest.raises(ffi.IsegmiError, match="libisegmi error -3: paint: an entry names a mask slot and the engine has no det.masks"):
            model.paint_device(image, e)
    finally:
        demo.close()


def test_engine_paint_needs_a_forward_and_masks_of_this_batch(ffi):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    lib = ffi.lib()
    model = MaskRCNN(maskrcnn_state_dict(1234), 192, 256, max_batch=1)
    try:
        image = _image(4, 150, 200)
        d = ffi.DeviceBuffer.from_numpy(image)
        box = np.array([[-1, 1, 1, 50, 40, 0x0000FF, 1, 0]], np.int32)
        tint = np.array([[0, 1, 1, 50, 40, 0x0000FF, 1, 0]], np.int32)
        for e in (box, tint):   # before any forward nothing is painted, slot or not
            assert lib.isegmi_engine_paint(model._h, 0, d.ptr, 150, 200, e.ctypes.data, 1, None, 0, d.ptr) == ERR_STATE
            assert lib.isegmi_last_error() == b"paint before forward"
        from isegmi.transforms import maskrcnn_resize_u8
        model([maskrcnn_resize_u8(image, 192, 256)])
        # after the forward: boxes paint, a slot has no det.masks of this batch until the paste ran
        assert lib.isegmi_engine_paint(model._h, 0, d.ptr, 150, 200, tint.ctypes.data, 1, None, 0, d.ptr) == ERR_STATE
        assert b"no det.masks of this batch" in lib.isegmi_last_error()
        model.sync()
        assert np.array_equal(d.numpy(), image)
        assert lib.isegmi_engine_paint(model._h, 0, d.ptr, 150, 200, None, 1, None, 0, d.ptr) == ERR_ARG
        import render_ref as R
        assert np.array_equal(model.paint_device(image, box), R.paint_ref(image, None, box, []))
        model.paste_device(150, 200, [(200, 150)])
        planes = None
        got = model.paint_device(image, tint)
        planes = model.fetch("det.masks", 1)[0]
        assert np.array_equal(got, R.paint_ref(image, planes, tint, []))
        # a list longer than one staging slot (4 KB = 128 entries), and the dot list's cap
        many = np.repeat(tint, 300, 0); many[:, 0] = np.arange(300) % 3; many[:, 5] = np.arange(300) * 0x010305 + 7
        dots = R.many_dots(3, 150, 200, 2000)
        assert np.array_equal(model.paint_device(image, many, dots), R.paint_ref(image, planes, many, dots))
        with pytest.raises(ffi.IsegmiError, match="Q <= 32768"):
            model.paint_device(image, box, np.zeros((32769, 4), np.int32))
    finally:
        model.close()


def _yolact(input_size=200, max_batch=2):
    """small frames resized up to the network size score 0.013 and below under the seeded weights: Detect's own cut goes from 0.05 to 0.005"""
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, YolactConfig
    return Yolact(yolact_state_dict(1234), cfg=dataclasses.replace(YolactConfig(), nms_conf_thresh=0.005), max_batch=max_batch, input_size=input_size)


@pytest.mark.parametrize("threshold,top_k", [(0.0, None), (0.0105, 15)])
def test_yolact_render_images_equals_overlay_of_postprocess(ffi, threshold, top_k):
    from isegmi.cli import _overlay
    from isegmi.yolact import postprocess, render_images
    frames = [_image(21, 120, 160), _image(22, 90, 131)]
    net = _yolact()
    try:
        for batch in ([frames[0]], frames):
            got = render_images(net, batch, threshold, top_k)
            assert len(got) == len(batch)
            out = net(batch)
            drawn = 0
            for i, im in enumerate(batch):
                h, w = im.shape[:2]
                classes, scores, boxes, masks = postprocess(out, w, h, i, threshold)
                classes, boxes, masks = classes[:top_k], boxes[:top_k], masks[:top_k]
                drawn += len(classes)
                want = _overlay(im, masks, boxes, classes)
                assert got[i].shape == im.shape and np.array_equal(got[i], want), "image %d of %d" % (i, len(batch))
                assert len(classes) == 0 or (want != im).any()
            print("yolact: %d detections drawn" % drawn)
            assert drawn >= 1, "the threshold of this test draws nothing: lower it"
    finally:
        net.close()


def test_eval_cli_render_device_writes_the_function_s_image(ffi, tmp_path):
    from PIL import Image
    from isegmi import cli
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, render_images
    frame = _image(2, 550, 550)   # noise at the network's own size: the default configuration's Detect keeps 100 candidates, up to 0.34
    src, dst = tmp_path / "in.png", tmp_path / "out.png"
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(src)
    args = cli.build_parser().parse_args(["eval"])
    assert not hasattr(args, "render")                       # the default is the host overlay: the flag leaves no attribute unless given
    cli.main(["eval", "--trained_model=random", "--score_threshold=0.15", "--top_k=15", "--image=%s:%s" % (src, dst), "--render=device", "--batch_size=1"])
    net = Yolact(yolact_state_dict(1234), max_batch=1)
    try:
        (want,) = render_images(net, [frame], 0.15, 15)
    finally:
        net.close()
    assert (want != frame).any(), "nothing was drawn: lower the threshold"
    assert np.array_equal(np.asarray(Image.open(dst).convert("RGB"))[:, :, ::-1], want)
