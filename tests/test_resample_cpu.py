"""The PIL-exact resize without a GPU: the numpy restatement against PIL itself, the library's host table builder against the
restatement, the geometry the front ends feed it, the refusals and the command line.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as rr


# ---------------------------------------------------------------------------------------------------------------- the reference against PIL
@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_restatement_equals_pil(shape):
    """Judges the reference: random bytes, the 0 / 255 board and all-255 at the ten shapes of the contract."""
    from PIL import Image
    h, w, oh, ow = shape
    for name, im in rr.patterns(h, w, seed=h * 7 + w).items():
        want = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR), np.uint8)
        got = rr.resize(im, oh, ow)
        assert got.shape == want.shape and np.array_equal(got, want), (shape, name, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------- the host table builder
def lib_tables(I, O):
    from isegmi import _ffi
    ks = C.c_int()
    _ffi.check(_ffi.lib().isegmi_resample_coeffs(I, O, None, None, C.byref(ks)))
    bounds, kk = np.full((O, 2), -7, np.int32), np.full((O, ks.value), -7, np.int32)
    _ffi.check(_ffi.lib().isegmi_resample_coeffs(I, O, bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p), C.byref(ks)))
    return bounds, kk


def check_axis(I, O):
    bounds, kk = lib_tables(I, O)
    rb, rk = rr.coeffs(I, O)
    assert kk.shape == rk.shape, (I, O, kk.shape, rk.shape)
    assert np.array_equal(bounds, rb) and np.array_equal(kk, rk), (I, O)


def test_coeffs_equal_the_restatement_small_sizes():
    """every (I, O) up to 40 x 40: upscales, downscales, I == O (one tap of 2^22), O == 1, I == 1"""
    for I in range(1, 41):
        for O in range(1, 41):
            check_axis(I, O)


@pytest.mark.parametrize("axis", [(480, 800), (640, 1067), (4000, 800), (427, 800), (640, 1199), (800, 800), (1333, 1333), (1, 1)])
def test_coeffs_equal_the_restatement_model_sizes(axis):
    check_axis(*axis)


def test_coeffs_identity_is_an_exact_copy():
    bounds, kk = lib_tables(57, 57)
    assert kk.shape == (57, 3)
    assert np.array_equal(bounds[:, 0], np.arange(57)) and np.array_equal(kk[:, 0], np.full(57, 1 << 22)) and not kk[:, 1:].any()


def test_coeffs_cap_and_refusals():
    from isegmi import _ffi
    from isegmi.transforms import RESAMPLE_MAX_KSIZE, resample_ksize, resample_tables
    assert RESAMPLE_MAX_KSIZE == rr.MAX_KSIZE == 1025
    check_axis(1024, 2)        # the largest downscale: 512, ksize 1025
    assert resample_ksize(1024, 2) == 1025 and lib_tables(1024, 2)[1].shape == (2, 1025)
    check_axis(512, 1)
    ks = C.c_int()
    for I, O in ((1025, 2), (513, 1)):   # one past the cap
        assert _ffi.lib().isegmi_resample_coeffs(I, O, None, None, C.byref(ks)) != 0
        assert b"ISEGMI_RESAMPLE_MAX_KSIZE" in _ffi.lib().isegmi_last_error()
        with pytest.raises(_ffi.IsegmiError, match="ISEGMI_RESAMPLE_MAX_KSIZE"):
            resample_tables(I, O)
    for I, O in ((0, 4), (4, 0), (-1, 3)):
        assert _ffi.lib().isegmi_resample_coeffs(I, O, None, None, C.byref(ks)) != 0
        assert b"I, O >= 1" in _ffi.lib().isegmi_last_error()


def test_resample_tables_are_cached_and_read_only():
    from isegmi.transforms import resample_tables
    a, b = resample_tables(33, 8), resample_tables(33, 8)
    assert a[0] is b[0] and a[1] is b[1]
    assert np.array_equal(a[0], rr.coeffs(33, 8)[0]) and np.array_equal(a[1], rr.coeffs(33, 8)[1])
    with pytest.raises(ValueError):
        a[1][0, 0] = 1


def dense(I, O):
    """The [O, I] integer matrix of an axis: row xx holds its taps at their source columns."""
    bounds, kk = lib_tables(I, O)
    M = np.zeros((O, I + kk.shape[1]), np.int64)
    np.put_along_axis(M, bounds[:, :1] + np.arange(kk.shape[1])[None], kk, 1)
    assert not M[:, I:].any()
    return M[:, :I]


def test_tables_are_mirror_symmetric_as_integers():
    """Why no view exists on which resize-then-mirror (upstream's order, the kernel's) and mirror-then-resize differ: the rounded 22-bit tables of an axis
    equal their own mirror image, for every (I, O) up to 48 and for the model's axes (an exhaustive search up to 400 found no exception either)."""
    pairs = [(I, O) for I in range(1, 49) for O in range(1, 49)] + [(480, 800), (640, 1067), (427, 800), (640, 1199), (4000, 800), (3000, 800), (1333, 800)]
    for I, O in pairs:
        M = dense(I, O)
        assert np.array_equal(M, M[::-1, ::-1]), (I, O)


# ---------------------------------------------------------------------------------------------------------------- geometry and the blob
def plan_entries(plan):
    """-> per view, per row: dict of the table words, with the tables read back OUT OF THE BLOB (what the kernel will read)."""
    from isegmi.transforms import RESAMPLE_ENTRY_WORDS
    head, tables = plan.header()
    words = head.view(np.int32)
    out = []
    for v, t in enumerate(tables):
        assert np.array_equal(words[plan.table_off[v] // 4:plan.table_off[v] // 4 + t.size].reshape(-1, RESAMPLE_ENTRY_WORDS), t)
        rows = []
        for w in t:
            co = words[plan.coeff_off // 4:]
            Hin, Win, Hout, Wout = (int(x) for x in w[2:6])
            bh = co[w[8]:w[8] + 2 * Wout].reshape(Wout, 2); kh = co[w[8] + 2 * Wout:w[8] + Wout * (2 + w[10])].reshape(Wout, w[10])
            bv = co[w[9]:w[9] + 2 * Hout].reshape(Hout, 2); kv = co[w[9] + 2 * Hout:w[9] + Hout * (2 + w[11])].reshape(Hout, w[11])
            rows.append(dict(src=int(w[0]), Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, dst=(int(w[6]), int(w[7])), hflip=int(w[12]), plane=int(w[13]),
                             h=(bh, kh), v=(bv, kv)))
        out.append(rows)
    return out


@pytest.mark.parametrize("hw", [(480, 640), (640, 427), (100, 100), (37, 91), (800, 1200), (300, 1900)])
def test_maskrcnn_geometry_feeds_the_tables_as_the_host_feeds_pil(hw):
    """The plan's (Hout, Wout) is what maskrcnn_resize_u8 hands PIL, its tables are the restatement's for exactly those axes, and the restatement on them
    equals the host path's bytes."""
    from isegmi.transforms import maskrcnn_resize_plan, maskrcnn_resize_u8
    rule = (64, 107)
    im = np.random.default_rng(hw[0]).integers(0, 256, hw + (3,), dtype=np.uint8)
    host = maskrcnn_resize_u8(im, *rule)
    plan, out_hw = maskrcnn_resize_plan([hw, hw], *rule)
    assert tuple(out_hw[0]) == host.shape[:2]
    (rows,) = plan_entries(plan)
    assert [r["src"] for r in rows] == [0, hw[0] * hw[1] * 3] and [r["plane"] for r in rows] == [0, 1]
    for r in rows:
        assert (r["Hin"], r["Win"], r["Hout"], r["Wout"]) == hw + host.shape[:2] and r["dst"] == (0, 0) and r["hflip"] == 0
        for (b, k), (I, O) in ((r["h"], (hw[1], host.shape[1])), (r["v"], (hw[0], host.shape[0]))):
            rb, rk = rr.coeffs(I, O)
            assert np.array_equal(b, rb) and np.array_equal(k, rk)
    assert np.array_equal(rr.resize(im, *host.shape[:2]), host)
    buf = np.zeros(plan.nbytes, np.uint8)
    plan.write(buf, [im, im])
    assert np.array_equal(buf[plan.src_off:plan.src_off + im.size], im.reshape(-1)) and np.array_equal(buf[plan.src_off + im.size:], im.reshape(-1))


@pytest.mark.parametrize("hw", [(120, 80), (80, 120), (64, 96), (500, 30)])
def test_letterbox_geometry_feeds_the_tables_as_the_host_feeds_pil(hw):
    """The YOLO epilogue of the restatement at letterbox_geometry's size and offsets equals yolo_letterbox on a non-square canvas."""
    from isegmi.transforms import letterbox_geometry, yolo_letterbox
    S_h, S_w = 64, 96
    im = np.random.default_rng(hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    want, (gain, px, py) = yolo_letterbox(im, S_h, S_w)
    g2, nh, nw, px2, py2 = letterbox_geometry(hw[0], hw[1], S_h, S_w)
    assert (gain, px, py) == (g2, px2, py2)
    got = rr.canvas_f32(im, nh, nw, S_h, S_w, py, px, (0, 0, 0), (255, 255, 255), True, 0.5)
    assert np.array_equal(rr.bits(got), rr.bits(want))


def test_bbox_aug_plan_views_follow_upstream_order():
    from isegmi.maskrcnn import BBoxAugConfig, MaskRCNNConfig, bbox_aug_plan, bbox_aug_views
    cfg = MaskRCNNConfig()
    aug = BBoxAugConfig(H_FLIP=True, SCALES=(48, 96), MAX_SIZE=160, SCALE_H_FLIP=True)
    sizes = [(60, 90), (90, 60)]
    plan, hws = bbox_aug_plan(sizes, cfg, aug, 64, 107)
    views = plan_entries(plan)
    assert len(views) == 6 and [[r["hflip"] for r in v] for v in views] == [[0, 0], [1, 1]] * 3
    for k, v in enumerate(views):
        for i, r in enumerate(v):
            assert (r["Hout"], r["Wout"], bool(r["hflip"])) == bbox_aug_views(sizes[i], cfg, aug, 64, 107)[k] and r["plane"] == i
            assert tuple(hws[k][i]) == (r["Hout"], r["Wout"])
    assert plan.pixel_bytes == sum(h * w * 3 for h, w in sizes)   # every original once, whatever the number of views


def test_plan_refuses_a_scale_beyond_the_cap():
    from isegmi.transforms import ResamplePlan
    with pytest.raises(ValueError, match="within 512"):
        ResamplePlan([(5130, 10)], [[(0, 10, 10, 0, 0, 0, 0)]])


# ---------------------------------------------------------------------------------------------------------------- refusals and the CLI
@pytest.mark.parametrize("argv, model", [(["eval", "--resize", "device"], "Yolact"),
                                         (["pose2seg_test", "--anno", "a.json", "--image-root", ".", "--resize", "device"], "Pose2Seg"),
                                         (["vit_classify", "--images", ".", "--resize", "device"], "ViT")])
def test_models_with_their_own_front_end_refuse_the_key_by_name(argv, model):
    from isegmi import cli
    assert cli.build_parser().parse_args(argv).resize == "device"
    with pytest.raises(SystemExit, match="--resize device: %s keeps its own front end" % model):
        cli.main(argv)


def test_python_interfaces_refuse_an_unknown_mode():
    from isegmi.maskrcnn import MaskRCNNConfig
    from isegmi.predictor import COCODemo
    from isegmi.yolov3 import YoloDetector
    with pytest.raises(ValueError, match="resize"):
        COCODemo(MaskRCNNConfig(), state_dict={}, resize="gpu")
    with pytest.raises(ValueError, match="resize"):
        YoloDetector({}, resize="gpu")


def test_cli_parses_resize():
    from isegmi import cli
    p = cli.build_parser()
    a = p.parse_args(["test_net", "--config-file", "configs/e2e_faster_rcnn_R_50_FPN_1x.yaml", "--resize", "device", "MODEL.WEIGHT", "random"])
    assert a.resize == "device" and a.opts == ["MODEL.WEIGHT", "random"]
    assert not hasattr(p.parse_args(["test_net"]), "resize")    # the default stays the host path
    y = p.parse_args(["yolo_detect", "--cfg", "configs/yolov3.cfg", "--images", "d", "--resize", "device"])
    assert y.resize == "device"
    assert not hasattr(p.parse_args(["yolo_detect", "--images", "d"]), "resize")
    with pytest.raises(SystemExit):
        p.parse_args(["test_net", "--resize", "gpu"])
