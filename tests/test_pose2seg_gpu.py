"""Pose2Seg on the MI355X: every pose-specific kernel through its op entry, and the whole forward, bit-exact against the CPU restatement
(tests/pose2seg_ref.py) on the same seeded weights; the COCO output of test() and the CLI; the refusals."""
import json

import numpy as np
import pytest

import pose2seg_ref as ref
from isegmi.weights import pose_templates

pytestmark = pytest.mark.gpu

SMALL = dict(width=32, blocks=(1, 1, 1, 1), fpn_channels=32, seg_width=32, seg_blocks=(2, 1))


def _kpts(rng, n, h, w, invisible=0.2):
    k = np.zeros((n, 17, 3), np.float32)
    cx, cy = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h
    for i in range(n):
        k[i, :, 0] = cx + rng.uniform(-0.25, 0.25, 17) * w
        k[i, :, 1] = cy + rng.uniform(-0.35, 0.35, 17) * h
        k[i, :, 2] = np.where(rng.uniform(size=17) < invisible, 0, 2)
    return k


def _dev(a):
    from isegmi import _ffi
    return _ffi.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("swap_rb,round_u8", [(0, 1), (1, 0)])
def test_letterbox_op_bitexact(ffi, swap_rb, round_u8):
    from isegmi.pose2seg import letterbox_inverse, letterbox_matrix
    rng = np.random.default_rng(swap_rb)
    imgs = [rng.integers(0, 256, hw + (3,), np.uint8) for hw in ((300, 700), (640, 200), (1, 1), (37, 53))]
    offs = np.cumsum([0] + [im.size for im in imgs])
    table = (ffi.P2sImage * len(imgs))()
    for n, im in enumerate(imgs):
        table[n].offset, table[n].h, table[n].w = int(offs[n]), im.shape[0], im.shape[1]
        table[n].minv[:] = letterbox_inverse(letterbox_matrix(*im.shape[:2]))
    d_u8 = _dev(np.concatenate([im.ravel() for im in imgs]))
    d_t = _dev(np.frombuffer(bytes(table), np.uint8))
    out = ffi.DeviceBuffer((len(imgs), 512, 512, 4))
    ffi.p2s_letterbox(d_u8, d_t, len(imgs), 512, ref.MEAN, ref.STD, swap_rb, round_u8, out)
    got = out.numpy()
    for n, im in enumerate(imgs):
        assert np.array_equal(got[n], ref.letterbox(im, swap_rb, round_u8)), n


def _fit_inputs(rng, R):
    from isegmi.weights import pose_templates
    hws = [(480, 640), (300, 200)]
    m1s = np.array([ref.m1_of(*hw) for hw in hws])
    roi_img = (np.arange(R) % 2).astype(np.int32)
    k = np.concatenate([_kpts(rng, 1, *hws[roi_img[r]]) for r in range(R)])
    k[1, :, 2] = 0                              # nothing visible
    k[2, 2:, 2] = 0                             # two visible
    k[3, :, 0] = k[3, :, 1] = 50; k[3, :, 2] = 2  # one place: collinear
    tp = pose_templates()
    return k, roi_img, m1s, tp


@pytest.mark.parametrize("align_corners", [0, 1])
def test_fit_op_bitexact(ffi, align_corners):
    rng = np.random.default_rng(5)
    R = 9
    k, roi_img, m1s, tp = _fit_inputs(rng, R)
    outs = [ffi.DeviceBuffer((R, 6)) for _ in range(3)] + [ffi.DeviceBuffer((R, 17, 3)), ffi.DeviceBuffer((R, 8), np.float64)]
    ffi.p2s_fit(_dev(k), _dev(roi_img), R, _dev(m1s), _dev(tp), tp.shape[0], align_corners, *outs)
    m3, G, mm, kal, fit = [o.numpy() for o in outs]
    ts = []
    for r in range(R):
        f = ref.fit(k[r], list(m1s[roi_img[r]]), tp, align_corners)
        assert np.array_equal(fit[r, :6], f["m3"]) and fit[r, 6] == f["err"] and fit[r, 7] == f["t"], r
        assert np.array_equal(m3[r], f["m3"].astype(np.float32)) and np.array_equal(G[r], f["G"]) and np.array_equal(mm[r], f["mmask"]), r
        assert np.array_equal(kal[r], f["kalign"]), r
        ts.append(f["t"])
    assert -1 in ts and max(ts) >= 0


@pytest.mark.parametrize("align_corners", [0, 1])
def test_align_and_skeleton_ops_bitexact(ffi, align_corners):
    rng = np.random.default_rng(7)
    R = 6
    k, roi_img, m1s, tp = _fit_inputs(rng, R)
    fits = [ref.fit(k[r], list(m1s[roi_img[r]]), tp, align_corners) for r in range(R)]
    feat = rng.standard_normal((2, 128, 128, 256)).astype(np.float32)
    G = np.stack([f["G"] for f in fits]); kal = np.stack([f["kalign"] for f in fits])
    G[0] = np.float32([1.3, 0.2, -5.0, -0.1, 1.2, 90.0])    # reaches past the map's border
    out = _dev(np.full((R, 64, 64, 320), np.nan, np.float32))
    d_ri = _dev(roi_img)
    ffi.p2s_align(_dev(feat), 128, 128, 256, d_ri, _dev(G), R, out, 320)
    ffi.p2s_skeleton(_dev(kal), R, out, 320, 256)
    got = out.numpy()
    for r in range(R):
        assert np.array_equal(got[r, ..., :256], ref.affine_align(feat[roi_img[r]], G[r])), r
        assert np.array_equal(got[r, ..., 256:311], ref.skeleton(kal[r])), r
        assert not got[r, ..., 311:].any()
    assert got[..., 256:273].max() == 1.0 and got[..., 273:311].any()


def test_masks_op_bitexact(ffi):
    rng = np.random.default_rng(9)
    hw = np.array([[50, 70], [90, 40], [20, 20]], np.int32)
    counts = np.array([2, 0, 3], np.int32)
    K = 4
    R = int(counts.sum())
    roi_off = np.array([0, 2, 2], np.int32)
    logits = rng.standard_normal((R, 64, 64, 2)).astype(np.float32) * 3
    mm = np.zeros((R, 6), np.float32)
    for r in range(R):
        s = rng.uniform(0.6, 2.5)
        mm[r] = (s, rng.uniform(-0.2, 0.2), rng.uniform(-20, 30), rng.uniform(-0.2, 0.2), s, rng.uniform(-20, 30))   # parts fall outside
    Hm, Wm = int(hw[:, 0].max()), int(hw[:, 1].max())
    masks = _dev(np.full((3, K, Hm, Wm), 7, np.uint8))
    boxes, scores = ffi.DeviceBuffer((3, K, 4)), ffi.DeviceBuffer((3, K))
    labels, cnt, ws = ffi.DeviceBuffer((3, K), np.int32), ffi.DeviceBuffer((3,), np.int32), ffi.DeviceBuffer((3, K, 4), np.int32)
    ffi.p2s_masks(_dev(logits), _dev(mm), _dev(counts), _dev(roi_off), _dev(hw), 3, K, Hm, Wm, ws, masks, boxes, scores, labels, cnt)
    M, B, S, L = masks.numpy(), boxes.numpy(), scores.numpy(), labels.numpy()
    assert list(cnt.numpy()) == list(counts) and M.any()
    for n in range(3):
        h, w = hw[n]
        for k in range(K):
            if k < counts[n]:
                m, b = ref.reverse_warp(logits[roi_off[n] + k], mm[roi_off[n] + k], h, w)
                assert np.array_equal(M[n, k, :h, :w], m) and np.array_equal(B[n, k], b) and S[n, k] == 1 and L[n, k] == 1, (n, k)
                assert not M[n, k, h:].any() and not M[n, k, :, w:].any()
            else:
                assert not M[n, k].any() and S[n, k] == 0 and L[n, k] == 0


def _images(rng):
    return [rng.integers(0, 256, hw + (3,), np.uint8) for hw in ((120, 200), (260, 90), (75, 75))]


@pytest.mark.parametrize("cat_skeleton,fpn_upsample,align_corners", [(1, "nearest", 0), (0, "bilinear", 1)])
def test_end_to_end_bitexact(ffi, cat_skeleton, fpn_upsample, align_corners):
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    cfg = Pose2SegConfig(cat_skeleton=cat_skeleton, fpn_upsample=fpn_upsample, align_corners=align_corners)
    sd = pose2seg_state_dict(11, cat_skeleton=bool(cat_skeleton), **SMALL)
    rng = np.random.default_rng(13)
    imgs = _images(rng)
    kmax = 3
    kps = [np.zeros((0, 17, 3), np.float32), _kpts(rng, 1, 260, 90), _kpts(rng, kmax, 75, 75)]
    kps[2][1, :, 2] = 0                         # one person with no visible keypoint
    net = Pose2Seg(sd, cfg, max_batch=3, max_instances=kmax)
    masks = net(imgs, kps, batchmasks=[None] * 3)
    L = net.last
    want = ref.forward(sd, imgs, kps, cfg)
    assert np.array_equal(net.read("p2", want["p2"].shape), want["p2"])
    assert np.array_equal(net.read("roi", want["roi"].shape), want["roi"])
    assert np.array_equal(net.read("logits", want["logits"].shape), want["logits"])
    _, boxes = net.collect()
    assert L["R"] == 4
    for n in range(3):
        assert len(masks[n]) == len(want["masks"][n]) == len(kps[n])
        for k in range(len(masks[n])):
            assert masks[n][k].shape == imgs[n].shape[:2]
            assert np.array_equal(masks[n][k], want["masks"][n][k]) and np.array_equal(boxes[n][k], want["boxes"][n][k]), (n, k)
    if cat_skeleton:   # these seeded weights give non-empty masks with the skeleton channels
        assert any(m.any() for ms in masks for m in ms)
    net.close()


def test_coco_output_and_cli(ffi, tmp_path):
    from PIL import Image
    from isegmi import cli
    from isegmi.coco import rle_encode
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig, test
    from isegmi.weights import pose2seg_state_dict
    sd = pose2seg_state_dict(1234, **SMALL)
    np.savez(tmp_path / "w.npz", **sd)
    rng = np.random.default_rng(17)
    imgs = [rng.integers(0, 256, (48, 64, 3), np.uint8), rng.integers(0, 256, (70, 30, 3), np.uint8)]
    kps = [_kpts(rng, 2, 48, 64), _kpts(rng, 1, 70, 30)]
    anno = {"images": [], "annotations": []}
    for i, (im, kp) in enumerate(zip(imgs, kps)):
        Image.fromarray(im[:, :, ::-1]).save(tmp_path / ("%d.png" % i))    # the CLI reads BGR like cv2.imread
        anno["images"].append({"id": 100 + i, "file_name": "%d.png" % i, "height": im.shape[0], "width": im.shape[1]})
        for k in kp:
            anno["annotations"].append({"image_id": 100 + i, "category_id": 1, "iscrowd": 0, "keypoints": k.ravel().tolist()})
    (tmp_path / "kp.json").write_text(json.dumps(anno))
    cfg = Pose2SegConfig()
    want = ref.forward(sd, imgs, kps, cfg)
    expect = [{"image_id": 100 + i, "category_id": 1, "segmentation": rle_encode(m), "score": 1.0,
               "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]}
              for i in range(2) for m, b in zip(want["masks"][i], want["boxes"][i])]
    assert any(m.any() for ms in want["masks"] for m in ms)
    net = Pose2Seg(sd, cfg, max_batch=2, max_instances=4)
    assert test(net, imgs, kps, [100, 101]) == expect
    assert test(net, imgs, kps, [100, 101], batch_size=1) == expect     # a short batch per step: padded record slots
    net.set_param("rle_cap_chars", 64.0)                                # the RLE overflows: the record loop grows the capacity and redoes the step
    net.set_param("rle_cap_runs", 1024.0)
    assert test(net, imgs, kps, [100, 101]) == expect
    net.close()
    out = tmp_path / "segm.json"
    cli.main(["pose2seg_test", "--weights", str(tmp_path / "w.npz"), "--anno", str(tmp_path / "kp.json"), "--image-root", str(tmp_path),
              "--output", str(out), "--batch-size", "2", "--max-instances", "4"])
    assert json.loads(out.read_text()) == expect


def test_refusals(ffi):
    from isegmi import _ffi
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    sd = pose2seg_state_dict(3, **SMALL)
    with pytest.raises(ValueError, match="fp16"):
        Pose2Seg(sd, Pose2SegConfig(fp16=True))
    with pytest.raises(ValueError, match="graph"):
        Pose2Seg(sd, Pose2SegConfig(graph=1))
    net = Pose2Seg(sd, Pose2SegConfig(), max_batch=1, max_instances=2)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (40, 40, 3), np.uint8)
    with pytest.raises(ValueError, match="max_instances"):
        net([img], [_kpts(rng, 3, 40, 40)])
    with pytest.raises(ValueError, match="17, 3"):
        net([img], [np.zeros((6, 17, 2), np.float32)])
    # the engine itself refuses too (ISEGMI_ERR_ARG with a message)
    d_u8 = _dev(img)
    d_k = _dev(_kpts(rng, 3, 40, 40))
    hw = np.array([40, 40], np.int32); cnt = np.array([3], np.int32)
    import ctypes as C
    fwd = lambda: _ffi.lib().isegmi_pose2seg_forward(net._h, d_u8.ptr, hw.ctypes.data_as(C.c_void_p), d_k.ptr, cnt.ctypes.data_as(C.c_void_p), 1)
    assert fwd() == -2 and b"more than max_instances = 2" in _ffi.lib().isegmi_last_error()
    cnt[0] = 1
    net.set_param("graph", 1.0)
    assert fwd() == -2 and b"graph" in _ffi.lib().isegmi_last_error()
    net.set_param("graph", 0.0)
    net.set_param("fp16", 1.0)
    assert fwd() == -2 and b"fp16" in _ffi.lib().isegmi_last_error()
    net.set_param("fp16", 0.0)
    assert fwd() == 0
    net.sync()
    net([img], [np.zeros((0, 17, 3), np.float32)])                     # no person: nothing stale to read
    with pytest.raises(ValueError, match="no person"):
        net.read("roi", (1, 64, 64, 96))
    net.close()
    with pytest.raises(_ffi.IsegmiError, match="template count"):
        _ffi.p2s_fit(None, None, 1, None, None, 65, 0, None, None, None, None, None)


def test_engine_records_kind3(ffi):
    """isegmi_engine_rle + isegmi_engine_pack_coco_records on a Pose2Seg engine: the Mask R-CNN record form with K = max_instances."""
    from isegmi import _ffi
    from isegmi.coco import rle_encode, results_from_records
    from isegmi.dist import unpack_coco_records
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    sd = pose2seg_state_dict(21, **SMALL)
    rng = np.random.default_rng(23)
    imgs = _images(rng)
    kps = [_kpts(rng, 2, 120, 200), np.zeros((0, 17, 3), np.float32), _kpts(rng, 1, 75, 75)]
    K = 5
    net = Pose2Seg(sd, Pose2SegConfig(), max_batch=4, max_instances=K)
    net.forward(imgs, kps)
    hw = [im.shape[:2] for im in imgs]
    net.rle_device(hw)
    nb, co = net.coco_record_bytes(4)
    dev = _ffi.DeviceBuffer((nb,), np.uint8)
    assert net.pack_coco_records(dev, 4) == nb
    net.sync()
    rec = unpack_coco_records(dev.numpy(), 4, K, 3, False, nb - co)
    want = ref.forward(sd, imgs, kps, Pose2SegConfig())
    assert list(rec["count"]) == [2, 0, 1, 0]
    for n in range(3):
        for k in range(len(kps[n])):
            assert np.array_equal(rec["box"][n, k], want["boxes"][n][k]) and rec["label"][n, k] == 1 and rec["score"][n, k] == 1.0
    res = results_from_records(rec, [5, 6, 7, None], hw + [(1, 1)], 3, K)
    assert [(d["image_id"], d["segmentation"]) for d in res] == [(i, rle_encode(m)) for i, ms in zip((5, 6, 7), want["masks"]) for m in ms]
    net.close()


# ---------------------------------------------------------------------------------------------------- paper widths, edges, capacity
def test_paper_widths_end_to_end_bitexact(ffi):
    """the default widths (ResNet-50 3-4-6-3, FPN 256, SegModule 10-1, a 320-channel RoI tensor); the test's own copy of the seeded
    weights moves segnet.conv_out.bias[1] so the masks are neither empty nor full"""
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    import pose2seg_fp64 as f64
    sd = dict(pose2seg_state_dict(11))
    rng = np.random.default_rng(29)
    imgs = [rng.integers(0, 256, hw + (3,), np.uint8) for hw in ((480, 640), (640, 427), (300, 301))]
    K = 8
    tp = pose_templates()
    kps = [f64.posed_persons(rng, 5, 480, 640, tp), f64.posed_persons(rng, K, 640, 427, tp), f64.posed_persons(rng, 6, 300, 301, tp)]
    cfg = Pose2SegConfig()
    net = Pose2Seg(sd, cfg, max_batch=3, max_instances=K)
    net.forward(imgs, kps)
    lg = net.read("logits", (19, 64, 64, 2))
    net.close()
    sd["segnet.conv_out.bias"] = sd["segnet.conv_out.bias"].copy()
    sd["segnet.conv_out.bias"][1] += np.float32(-np.median(lg[..., 1] - lg[..., 0]))
    net = Pose2Seg(sd, cfg, max_batch=3, max_instances=K)
    masks = net(imgs, kps)
    _, boxes = net.collect()
    want = ref.forward(sd, imgs, kps, cfg)
    for name in ("p2", "roi", "logits"):
        assert np.array_equal(net.read(name, want[name].shape), want[name]), name
    fg = (want["logits"][..., 1] > want["logits"][..., 0]).mean()
    assert 0.1 < fg < 0.9, fg
    for n in range(3):
        for k in range(len(kps[n])):
            assert np.array_equal(masks[n][k], want["masks"][n][k]) and np.array_equal(boxes[n][k], want["boxes"][n][k]), (n, k)
    assert all(m.any() and not m.all() for ms in masks for m in ms)
    net.close()


@pytest.mark.parametrize("T,align_corners", [(1, 0), (64, 1), (3, 0)])
def test_fit_edges_bitexact(ffi, T, align_corners):
    """T = 1 / 64 (random templates, some zero-weight joints, a duplicate), v in {-1, 1, 2}, +-1e5, duplicated persons, off-frame and
    non-finite keypoints, R = 256"""
    import pose2seg_fp64 as f64
    import pose2seg_run as run
    rng = np.random.default_rng(200 + T)
    hws = [(480, 640), (333, 200), (1, 1)]
    e = f64.edge_persons(rng, *hws[0])
    k = np.concatenate([e, f64.persons(rng, 256 - len(e), *hws[1], invisible=0.3)])
    k[-15:-10] = k[-20:-15]                                       # duplicated persons (one image)
    roi_img = np.array([0] * len(e) + [1] * (256 - len(e) - 3) + [2] * 3, np.int32)
    tp = pose_templates() if T == 3 else f64.random_templates(rng, T)
    m3, G, mm, kal, fit = run.fit(ffi, k, roi_img, hws, tp, align_corners)
    ts = []
    for r in range(len(k)):
        f = ref.fit(k[r], list(f64.m1_matrix(*hws[roi_img[r]])[:2].ravel()), tp, align_corners)
        assert np.array_equal(fit[r, :6], f["m3"]) and fit[r, 6] == f["err"] and fit[r, 7] == f["t"], r
        assert np.array_equal(G[r], f["G"]) and np.array_equal(mm[r], f["mmask"]) and np.array_equal(kal[r], f["kalign"], equal_nan=True), r
        ts.append(f["t"])
    assert -1 in ts and max(ts) >= 0
    assert np.array_equal(fit[-15:-10], fit[-20:-15])


def test_nonfinite_keypoints_fit_bitexact(ffi):
    """a NaN / inf coordinate counts as not visible on the GPU as in the restatement: the fallback box of [NaN, one finite point] is the
    8 px box of the finite point, not NaN and not a box stretched by the NaN"""
    import pose2seg_run as run
    k = np.zeros((3, 17, 3), np.float32)
    k[0, 0] = (np.nan, 100, 2); k[0, 1] = (200, 120, 2)
    k[1, 0] = (np.inf, 100, 2); k[1, 1] = (200, 120, 2); k[1, 2] = (210, -np.inf, 2)
    k[2, :, :2] = np.random.default_rng(1).uniform(50, 400, (17, 2)); k[2, :, 2] = 2; k[2, 4, 0] = np.nan
    hws = [(480, 640)]
    tp = pose_templates()
    m3, G, mm, kal, fit = run.fit(ffi, k, np.zeros(3, np.int32), hws, tp, 0)
    for r in range(3):
        f = ref.fit(k[r], ref.m1_of(*hws[0]), tp, 0)
        assert np.array_equal(fit[r, :6], f["m3"]) and fit[r, 7] == f["t"] and np.array_equal(G[r], f["G"]), r
        assert np.all(np.isfinite(fit[r, :6])) and np.all(np.isfinite(mm[r])), r
        assert np.array_equal(kal[r], f["kalign"], equal_nan=True)
    assert fit[0, 7] == fit[1, 7] == -1 and fit[0, 0] == fit[1, 0] == 8.0 and fit[2, 7] >= 0
    assert kal[0, 0, 2] == 0 and kal[1, 2, 2] == 0 and kal[2, 4, 2] == 0 and kal[0, 1, 2] == 2


def test_align_edges_bitexact(ffi):
    """C = 4 and C = 256 into a wider row (out_c > C, no skeleton: channels past C untouched); samples exactly on -1, 0, W - 1 and W;
    a NaN matrix samples nothing"""
    import pose2seg_run as run
    rng = np.random.default_rng(210)
    G = np.float32([[1, 0, -1, 0, 1, 64], [1, 0, 65, 0, 1, -1], [0.5, 0, 0, 0, 0.5, 0], [np.nan] * 6, [1, 0, 64.5, 0, 1, 63.5]])
    roi_img = np.array([0, 1, 0, 1, 0], np.int32)
    for C, out_c in ((4, 4), (256, 320), (8, 12)):
        feat = rng.standard_normal((2, 128, 128, C)).astype(np.float32)
        got = run.align_skeleton(ffi, feat, roi_img, G, None, out_c, skeleton=False, fill=-7.0)
        for r in range(len(G)):
            assert np.array_equal(got[r, ..., :C], ref.affine_align(feat[roi_img[r]], G[r])), (C, r)
        assert np.all(got[..., C:] == -7.0)
        assert not got[3, ..., :C].any()


def test_skeleton_edges_bitexact(ffi):
    """zero-length and axis-aligned limbs, joints outside [0, 64), pixels at |perp| = 1 exactly and at e = 4.6052"""
    import pose2seg_run as run
    kal = np.zeros((4, 17, 3), np.float32)
    kal[..., 2] = 2
    kal[0, :, :2] = np.random.default_rng(3).uniform(-30, 94, (17, 2))            # many joints off the frame
    kal[1, :, :2] = (30.0, 30.0)                                                      # every limb zero-length
    kal[2, 5, :2] = (30.0, 10.0); kal[2, 6, :2] = (30.0, 50.0)                       # vertical: columns 29 / 31 at |perp| = 1
    kal[2, 11, :2] = (10.0, 40.0); kal[2, 12, :2] = (55.0, 40.0)                     # horizontal
    kal[2, 0, :2] = (np.float32(32.0) + np.float32(np.sqrt(2 * 9 * 4.6052)), 5.0)      # a pixel at the heatmap cut
    kal[3, :, :2] = (-5.0, 70.0); kal[3, 0, :2] = (-0.5, 64.5)
    got = run.align_skeleton(ffi, np.zeros((1, 128, 128, 4), np.float32), np.zeros(4, np.int32), np.zeros((4, 6), np.float32), kal, 68)
    for r in range(4):
        assert np.array_equal(got[r, ..., 4:59], ref.skeleton(kal[r])), r
        assert not got[r, ..., 59:].any()
    l = ref.LIMBS.index([6, 7])
    assert got[2, 10:50, 30, 4 + 18 + 2 * l].all() and not got[2, :, 29, 4 + 17 + 2 * l:4 + 19 + 2 * l].any()


def test_masks_edges_bitexact(ffi):
    """N K = 65535 accepted and 65536 refused (tiny planes); Hmax and Wmax from different images, not multiples of 64; a 1 x 1 and a
    3000 x 4000 image; logits of +-inf, NaN, equal pairs (p = 0.5 gives 0) and +-1e30"""
    import pose2seg_run as run
    from isegmi import _ffi
    rng = np.random.default_rng(220)
    lg = rng.standard_normal((3, 64, 64, 2)).astype(np.float32) * 3
    mm = np.float32([[0.6, 0, 1, 0, 0.6, 2]] * 3)
    M, B, S, L, cnt = run.masks(ffi, lg, mm, [1, 0, 2], [(1, 1), (2, 1), (1, 2)], 21845)
    assert M.shape == (3, 21845, 2, 2) and list(cnt) == [1, 0, 2] and S[0, 0] == 1 and S[0, 1] == 0 and not M[0, 1:].any()
    with pytest.raises(_ffi.IsegmiError, match="65535"):
        run.masks(ffi, lg, mm, [1, 0], [(1, 1), (1, 1)], 32768)
    special = rng.standard_normal((64, 64, 2)).astype(np.float32) * 1e30
    special[:8] = np.inf; special[8:16, :, 0] = -np.inf; special[16:24, :32] = np.nan; special[24:40] = special[24:40, :, :1]   # equal pairs
    special[40:48, :, 1] = -np.inf
    lg = np.stack([special, lg[0], lg[1], lg[2]])
    hw = np.array([[70, 30], [20, 130], [1, 1]], np.int32)
    mm = np.float32([[0.9, 0.1, -2, -0.1, 0.9, 3], [1.5, 0, -10, 0, 1.5, 5], [0.5, 0, 0, 0, 0.5, 0], [64, 0, 0, 0, 64, 0]])
    counts = np.array([2, 1, 1], np.int32)
    M, B, S, L, cnt = run.masks(ffi, lg, mm, counts, hw, 3)
    assert M.shape == (3, 3, 70, 130)
    r = 0
    for n in range(3):
        h, w = hw[n]
        for k in range(3):
            if k < counts[n]:
                m, b = ref.reverse_warp(lg[r], mm[r], h, w)
                assert np.array_equal(M[n, k, :h, :w], m) and np.array_equal(B[n, k], b), (n, k)
                r += 1
            assert not M[n, k, h:].any() and not M[n, k, :, w:].any()
    eq = np.full((1, 64, 64, 2), -2.5, np.float32)
    M, B, *_ = run.masks(ffi, eq, np.float32([[1, 0, 0, 0, 1, 0]]), [1], [(64, 64)], 1)
    assert not M.any() and not B.any()
    big = np.zeros((1, 64, 64, 2), np.float32); big[0, 20:40, 10:50, 1] = 4
    h, w = 3000, 4000
    M, B, *_ = run.masks(ffi, big, np.float32([[64 / 4000, 0, 0, 0, 64 / 4000, 0]]), [1], [(h, w)], 2)
    m, b = ref.reverse_warp(big[0], np.float32([64 / 4000, 0, 0, 0, 64 / 4000, 0]), h, w)
    assert np.array_equal(M[0, 0], m) and np.array_equal(B[0, 0], b) and m.any() and not M[0, 1].any()


def test_engine_back_to_back_changing_R(ffi):
    """one engine, forwards with R = 7, 1, 0, max_batch * K (full capacity), 3: each equal to the restatement (stale or under-sized
    reused buffers would show)"""
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    import pose2seg_fp64 as f64
    sd = pose2seg_state_dict(41, **SMALL)
    cfg = Pose2SegConfig()
    K = 4
    net = Pose2Seg(sd, cfg, max_batch=2, max_instances=K)
    rng = np.random.default_rng(43)
    for counts in ((4, 3), (1, 0), (0, 0), (K, K), (2, 1)):
        imgs = [rng.integers(0, 256, (int(rng.integers(20, 200)), int(rng.integers(20, 200)), 3), np.uint8) for _ in counts]
        kps = [f64.persons(rng, c, *im.shape[:2]) for c, im in zip(counts, imgs)]
        masks = net(imgs, kps)
        _, boxes = net.collect()
        want = ref.forward(sd, imgs, kps, cfg)
        assert net.last["R"] == sum(counts)
        assert np.array_equal(net.read("p2", want["p2"].shape), want["p2"])
        if sum(counts):
            assert np.array_equal(net.read("roi", want["roi"].shape), want["roi"])
            assert np.array_equal(net.read("logits", want["logits"].shape), want["logits"])
        for n in range(2):
            assert len(masks[n]) == counts[n]
            for k in range(counts[n]):
                assert np.array_equal(masks[n][k], want["masks"][n][k]) and np.array_equal(boxes[n][k], want["boxes"][n][k]), (counts, n, k)
        assert list(net.read("count", (2,), np.int32)) == list(counts)
    net.close()
