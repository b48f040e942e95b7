"""The painter's contract without a GPU: tests/render_ref.paint_ref IS the host overlays (COCODemo.overlay, overlay_keypoints, cli._overlay) when it is
fed the draw lists of isegmi.render, its integer blend is their float blend for every byte pair, and the shared cases tell apart the mistakes a
pixel-parallel painter can make (order, tint / outline order, what counts as a set mask byte)."""
import numpy as np
import pytest

import render_ref as R
from isegmi import render
from isegmi.cli import _overlay
from isegmi.predictor import COCODemo


def test_integer_blend_is_the_float_blend_for_every_byte_pair():
    p, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    host = (0.5 * p + 0.5 * c.astype(np.float32)).astype(np.uint8)      # image[m] = (0.5 * image[m] + 0.5 * c).astype(np.uint8)
    assert host.shape == (256, 256)
    assert np.array_equal(host, ((p.astype(np.uint16) + c) >> 1).astype(np.uint8))
    # the packed form the kernel uses: three bytes of a register at once, no carry between them
    pp = p.astype(np.uint32) * 0x010101; cc = c.astype(np.uint32) * 0x010101
    packed = (pp & cc) + (((pp ^ cc) & 0xFEFEFE) >> 1)
    assert np.array_equal(packed, host.astype(np.uint32) * 0x010101)


@pytest.fixture()
def demo(monkeypatch):
    d = COCODemo(None, confidence_threshold=0.5, state_dict={"unused": None})
    monkeypatch.setattr(COCODemo, "overlay_class_names", lambda self, image, predictions: image)   # the text step stays on the host, after the painter
    return d


@pytest.mark.parametrize("H,W,n", [(23, 37, 6), (5, 63, 3), (40, 31, 12), (9, 9, 0)])
def test_restatement_equals_cocodemo_overlay(demo, H, W, n):
    rng = np.random.default_rng(H * W)
    image = R.random_image(rng, H, W)
    pred = R.crafted_predictions(7 + n, H, W, n)
    want = demo.overlay(image.copy(), pred)
    ph, pw = R.plane_shape(H, W, 3)
    got = R.paint_ref(image, R.slot_planes(pred, ph, pw), render.demo_entries(pred, H, W), None)
    assert np.array_equal(got, want)
    if n:
        assert not np.array_equal(want, image)


def test_restatement_equals_box_only_overlay(demo):
    H, W, n = 19, 33, 5
    image = R.random_image(np.random.default_rng(3), H, W)
    pred = R.crafted_predictions(11, H, W, n, with_masks=False)
    want = demo.overlay(image.copy(), pred)
    e = render.demo_entries(pred, H, W, with_masks=False)
    assert (e[:, 0] == -1).all()
    assert np.array_equal(R.paint_ref(image, None, e, []), want) and not np.array_equal(want, image)


def test_restatement_equals_overlay_keypoints(demo):
    H, W, n = 31, 45, 4
    image = R.random_image(np.random.default_rng(5), H, W)
    pred = R.crafted_predictions(13, H, W, n, keypoints=True, with_masks=False)
    pred.get_field("keypoint_logits")[0, :2] = 3.0   # the two corner dots are drawn
    want = demo.overlay(image.copy(), pred)          # boxes, then overlay_keypoints
    dots = render.keypoint_dots(pred, demo.KP_THRESH)
    assert 2 <= len(dots) < n * 17 and (dots[:, 3] == 2).all()
    got = R.paint_ref(image, None, render.demo_entries(pred, H, W, with_masks=False), dots)
    assert np.array_equal(got, want)
    only = demo.overlay_keypoints(image.copy(), pred)
    assert np.array_equal(R.paint_ref(image, None, [], dots), only) and not np.array_equal(only, image)


@pytest.mark.parametrize("H,W,n", [(30, 41, 5), (12, 64, 2)])
def test_restatement_equals_cli_overlay(H, W, n):
    rng = np.random.default_rng(H + W)
    image = R.random_image(rng, H, W)
    pred = R.crafted_predictions(17, H, W, n)
    masks = pred.get_field("mask")[:, 0]
    boxes = np.maximum(pred.bbox, 0).astype(np.int64)   # postprocess() boxes: integers, never negative, x2 / y2 up to W / H
    boxes[0, 2:] = (W, H)
    classes = pred.get_field("labels") - 1
    want = _overlay(image, masks, boxes, classes)
    ph, pw = R.plane_shape(H, W, 1)
    got = R.paint_ref(image, R.planes_of(masks, ph, pw), render.yolact_entries(np.arange(n), boxes, classes, H, W), [])
    assert np.array_equal(got, want) and not np.array_equal(want, image)


def test_builders_give_the_host_integers():
    H, W = 20, 30
    pred = R.crafted_predictions(19, H, W, 4)
    pred.bbox[0] = (-2.7, -0.2, 40.9, 19.99)
    pred.bbox[1] = (3.99, 4.01, 3.2, 25.0)
    e = render.demo_entries(pred, H, W)
    assert e.dtype == np.int32 and e.shape == (4, 8)
    assert e[0, 1:5].tolist() == [0, 0, 29, 19] and e[1, 1:5].tolist() == [3, 4, 3, 19]   # int() truncates, then both corners clamp into the image
    assert e[:, 0].tolist() == pred.get_field("slot").tolist() and (e[:, 6] == 1).all() and (e[:, 7] == 0).all()
    col = COCODemo.compute_colors_for_labels(pred.get_field("labels"))
    assert [R.unpack_color(int(c)).tolist() for c in e[:, 5]] == col.tolist()
    y = render.yolact_entries([2, 0], np.array([[1, 2, 30, 20], [0, 0, 5, 5]]), np.array([0, 79]), H, W)
    assert y[:, :5].tolist() == [[2, 1, 2, 29, 19], [0, 0, 0, 5, 5]]            # only x2 / y2 clamp, to W-1 / H-1
    assert R.unpack_color(int(y[1, 5])).tolist() == COCODemo.compute_colors_for_labels([80])[0].tolist()   # colours of class + 1
    kp = R.crafted_predictions(23, H, W, 2, keypoints=True, with_masks=False)
    kp.get_field("keypoint_logits")[:] = 0.0
    kp.get_field("keypoint_logits")[1, 16] = 2.5
    kp.get_field("keypoints")[1, 16] = (7.9, 8.2, 1.0)
    d = render.keypoint_dots(kp, 2.0)
    assert d.tolist() == [[7, 8, int(render.pack_colors(COCODemo.compute_colors_for_labels([17]))[0]), 2]]
    with pytest.raises(ValueError):
        render.make_entries(np.zeros(1025), np.zeros((1025, 4)), np.zeros((1025, 3)))


def test_cli_flags_and_render_keyword():
    from isegmi.cli import build_parser
    ap = build_parser()
    assert not hasattr(ap.parse_args(["eval"]), "render") and ap.parse_args(["eval", "--render=device"]).render == "device"
    t = ap.parse_args(["test_net", "--vis-dir", "out", "--render", "device", "--vis-threshold", "0.3"])
    assert (t.vis_dir, t.render, t.vis_threshold) == ("out", "device", 0.3)
    assert not {"vis_dir", "render", "vis_threshold"} & set(vars(ap.parse_args(["test_net"])))
    with pytest.raises(SystemExit):
        ap.parse_args(["eval", "--render", "gpu"])
    assert COCODemo(None, state_dict={"unused": None}).render == "host"
    assert COCODemo(None, state_dict={"unused": None}, render="device").render == "device"
    with pytest.raises(ValueError, match="render"):
        COCODemo(None, state_dict={"unused": None}, render="gpu")


def test_cases_discriminate():
    H, W = 7, 67
    image, masks, e, (cx, cy) = R.overlap_case(1, H, W, 1, 2)
    e[:, 0] = (0, 1); e[:, 6] = 0; e[0, 5], e[1, 5] = 0x0000FF, 0xFF0000
    a, b = R.paint_ref(image, masks, e, []), R.paint_ref(image, masks, e[::-1], [])
    assert not np.array_equal(a[cy, cx], b[cy, cx])                       # painter's order: swapping two overlapping entries shows
    # an outline that a FOLLOWING mask tints is not tint-then-outline
    masks[:] = 1
    first = np.array([[-1, 0, 0, W - 1, H - 1, 0x00FF00, 1, 0], [0, 0, 0, 0, 0, 0x0000FF, 0, 0]], np.int32)
    one = np.array([[0, 0, 0, W - 1, H - 1, 0x0000FF, 0, 0], [-1, 0, 0, W - 1, H - 1, 0x00FF00, 1, 0]], np.int32)
    assert not np.array_equal(R.paint_ref(image, masks, first, [])[0, 0], R.paint_ref(image, masks, one, [])[0, 0])
    # within ONE entry the tint comes before the outline: the outline pixel shows the pure colour
    both = np.array([[0, 0, 0, W - 1, H - 1, 0x0000FF, 1, 0]], np.int32)
    assert R.paint_ref(image, masks, both, [])[0, 0].tolist() == [255, 0, 0]
    # a mask byte of 2 (or 255) is set, 0 is not
    masks[:] = 0
    masks[0, 1, 1], masks[0, 1, 2] = 2, 255
    t = R.paint_ref(image, masks, np.array([[0, 0, 0, 0, 0, 0x123456, 0, 0]], np.int32), [])
    changed = np.nonzero((t != image).any(2))
    assert set(zip(*changed)) <= {(1, 1), (1, 2)} and np.array_equal(t[1, 1], (image[1, 1].astype(int) + [0x56, 0x34, 0x12]) >> 1)
    # y2 < y1 still paints rows y1 and y2, and no column
    name, ent = R.outline_entries(H, W)[4]
    o = R.paint_ref(np.zeros((H, W, 3), np.uint8), None, [ent], [])
    assert name == "y2 < y1" and o[0].any(1).all() and o[H - 1].any(1).all() and not o[1:H - 1].any()
    for name, ent in R.outline_entries(H, W):
        painted = R.paint_ref(np.zeros((H, W, 3), np.uint8), None, [ent], []).any()
        assert painted == (not name.startswith(("outside", "spans", "flag off"))), name
    for name, dots in R.dot_cases(H, W):
        o = R.paint_ref(np.zeros((H, W, 3), np.uint8), None, [], dots)
        half = int(dots[0, 3])
        assert o.any() == (not (name.startswith("outside half 0") or name == "just out of reach")), name
        if name.startswith("corners"):
            assert o[0, 0].any() and o[H - 1, W - 1].any() and (o.any(2).sum() <= 4 * (half + 1) ** 2)
