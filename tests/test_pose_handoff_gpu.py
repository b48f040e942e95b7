"""Keypoint R-CNN -> Pose2Seg on the device: the hand-off kernel against its numpy restatement on the cases of
tests/pose_handoff_cases.py, the hand-off of a real Keypoint R-CNN forward against the keypoint record block, and the whole KeypointPose2Seg pipeline
against the host composition MaskRCNN.__call__ -> restatement -> Pose2Seg.forward.  Every comparison is bit for bit."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

import pose_handoff_cases as cases
import pose_handoff_ref as ref
from conv_ref import same_bits

pytestmark = pytest.mark.gpu

SCORE_THRESH = 0.012   # as tests/test_keypointrcnn_gpu.py: the seeded two-class predictor keeps its 81-class background bias
SMALL = dict(width=32, blocks=(1, 1, 1, 1), fpn_channels=32, seg_width=32, seg_blocks=(2, 1))
MIN_SIZE, MAX_SIZE = 96, 160   # the detector's resize of the end-to-end images: 150 x 200 -> 96 x 128, ratios != 1


# ------------------------------------------------------------------------------------------------------------ the op against the restatement
@pytest.mark.parametrize("name", sorted(cases.all_cases()))
def test_op_equals_the_restatement(ffi, name):
    c = cases.all_cases()[name]
    N, K = c["score"].shape[0], c["K"]
    want = ref.handoff(**c)
    kp, sc, sl, cnt = ffi.pose_handoff(c["score"], c["count"], c["kpt"], c["kscore"], c["ratios"], c["person_thresh"], c["kp_thresh"], K)
    R = int(want[3].sum())
    assert cnt.tolist() == want[3].tolist(), name
    assert same_bits(sc, want[1]) and np.array_equal(sl, want[2]), name
    assert kp.shape == (N * K, 17, 3) and same_bits(kp[:R], want[0]), name
    assert (kp[R:].view(np.uint8) == 0xFF).all(), "rows behind the last person were written"
    assert np.isfinite(kp[:R]).all() and np.isfinite(sc).all()                         # nothing of the garbage behind the counts came through


def test_op_refuses_other_keypoint_counts_by_name(ffi):
    c = cases.single_case()
    with pytest.raises(ffi.IsegmiError, match="num_keypoints"):
        ffi.pose_handoff(c["score"], c["count"], np.zeros((1, 1, 16, 3), np.float32), np.zeros((1, 1, 16), np.float32), c["ratios"], 0.5, 2.0, 1)


# ------------------------------------------------------------------------------------------------------------ through the Keypoint R-CNN engine
def _cfg(**kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return dataclasses.replace(MaskRCNNConfig(), **{**dict(MASK_ON=False, NUM_CLASSES=2, KEYPOINT_ON=True, ROI_SCORE_THRESH=SCORE_THRESH), **kw})


@functools.lru_cache(maxsize=None)
def _sd():
    from isegmi.weights import keypointrcnn_state_dict
    return keypointrcnn_state_dict(1234)


@functools.lru_cache(maxsize=None)
def _batch():
    """Three images on the 128 x 160 canvas (the batch of tests/test_keypointrcnn_gpu.py)."""
    from isegmi.maskrcnn import prepare_images
    rng = np.random.default_rng(20261019)
    x, hw = prepare_images([rng.uniform(0, 255, s).astype(np.float32) for s in ((100, 130, 3), (120, 150, 3), (128, 101, 3))])
    assert x.shape[1:3] == (128, 160)
    x.setflags(write=False)
    return x, hw


@pytest.fixture(scope="module")
def detector(ffi):
    from isegmi.maskrcnn import MaskRCNN
    m = MaskRCNN(_sd(), 128, 160, cfg=_cfg(MIN_SIZE_TEST=MIN_SIZE, MAX_SIZE_TEST=MAX_SIZE), max_batch=3)
    yield m
    m.close()


def _handoff_buffers(ffi, N, K):
    return [ffi.DeviceBuffer((N * K, 17, 3)).poison(), ffi.DeviceBuffer((N, K)).poison(), ffi.DeviceBuffer((N, K), np.int32).poison(),
            ffi.DeviceBuffer((N,), np.int32).poison()]


def _middle(values):
    """a threshold strictly between two neighbouring distinct values around the median: some pass, some do not"""
    v = np.unique(np.asarray(values, np.float32))
    assert len(v) >= 2, "the detector's scores are all equal"
    i = len(v) // 2
    return float((np.float64(v[i - 1]) + np.float64(v[i])) / 2)


def test_engine_handoff_equals_the_keypoint_records(ffi, detector):
    from isegmi.dist import unpack_coco_records
    m = detector
    x, hw = _batch()
    m.upload(x, hw)
    m.forward_device(3)
    sizes = [(333, 517), (160, 128), (77, 401)]
    m.set_output_sizes(sizes)
    nb = m.coco_record_bytes(3)[0]
    dev = ffi.DeviceBuffer((nb,), np.uint8)
    assert m.pack_keypoint_records(dev, 3) == nb
    m.sync()
    rec = unpack_coco_records(dev.numpy(), 3, 100, 2, box_only=True, keypoints=17)
    det = {k: m.fetch(k, 3).copy() for k in ("det.score", "det.count", "det.kpt", "det.kscore")}
    cnt = det["det.count"]
    live = np.concatenate([det["det.score"][n, :cnt[n]] for n in range(3)])
    print("detections per image:", cnt.tolist())
    thr = _middle(live)
    kthr = _middle(np.concatenate([det["det.kscore"][n, :cnt[n]].ravel() for n in range(3)]))
    K = 4
    outs = _handoff_buffers(ffi, 3, K)
    ratios = m.pose_handoff(thr, kthr, K, *outs)
    m.sync()
    kp, sc, sl, co = (o.numpy() for o in outs)
    want = ref.handoff(det["det.score"], cnt, det["det.kpt"], det["det.kscore"], ratios, thr, kthr, K)
    R = int(co.sum())
    print("persons per image:", co.tolist(), "of candidates", [(det["det.score"][n, :cnt[n]] > np.float32(thr)).sum() for n in range(3)])
    assert 0 < R < int(cnt.sum()) and (ratios != 1).all()
    assert co.tolist() == want[3].tolist() and same_bits(sc, want[1]) and np.array_equal(sl, want[2]) and same_bits(kp[:R], want[0])
    assert (kp[R:].view(np.uint8) == 0xFF).all()
    r = 0
    for n in range(3):                      # the rows against the record block's kpt rows, joined through src_slot
        for k in range(int(co[n])):
            j = int(sl[n, k])
            assert same_bits(kp[r, :, :2], rec["kpt"][n, j, :, :2]) and sc[n, k] == rec["score"][n, j], (n, k, j)
            assert np.array_equal(kp[r, :, 2], np.where(rec["kscore"][n, j] > np.float32(kthr), 2, 0).astype(np.float32)), (n, k, j)
            r += 1
    assert set(np.unique(kp[:R, :, 2]).tolist()) == {0.0, 2.0}


def test_engine_refusals_name_their_cause(ffi, detector):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    outs = _handoff_buffers(ffi, 1, 2)
    fresh = MaskRCNN(_sd(), 128, 160, cfg=_cfg(), max_batch=1)
    try:
        with pytest.raises(ffi.IsegmiError, match="before forward"):
            fresh.pose_handoff(0.5, 2.0, 2, *outs)
    finally:
        fresh.close()
    box = MaskRCNN(maskrcnn_state_dict(1234, mask=False, num_classes=2), 128, 160, cfg=_cfg(KEYPOINT_ON=False), max_batch=1)
    try:
        x, hw = _batch()
        box.upload(x[:1], hw[:1]); box.forward_device(1); box.sync()
        with pytest.raises(ffi.IsegmiError, match="keypoint_on 0"):
            box.pose_handoff(0.5, 2.0, 2, *outs)
        from isegmi.pose2seg import KeypointPose2Seg
        with pytest.raises(ValueError, match="KEYPOINT_ON"):
            KeypointPose2Seg(box, None)
    finally:
        box.close()


# ------------------------------------------------------------------------------------------------------------ end to end
def _images():
    from conftest import smooth_field
    rng = np.random.default_rng(41)
    return [rng.integers(0, 256, (150, 200, 3)).astype(np.uint8), np.ascontiguousarray(smooth_field(7, 200, 150), np.uint8),
            rng.integers(0, 256, (150, 200, 3)).astype(np.uint8)]


@pytest.fixture(scope="module")
def p2s_sd():
    from isegmi.weights import pose2seg_state_dict
    return pose2seg_state_dict(11, **SMALL)


@pytest.fixture(scope="module")
def detections(detector):
    """The detector's own answer on the three images, through MaskRCNN.__call__ (sync, fetches, BoxLists): padded to [N, cap] arrays + the ratios"""
    from isegmi.transforms import maskrcnn_resize_u8
    images = _images()
    bls = detector([maskrcnn_resize_u8(im, MIN_SIZE, MAX_SIZE) for im in images])
    N, cap = len(images), 100
    d = dict(score=np.zeros((N, cap), np.float32), count=np.zeros(N, np.int32), kpt=np.zeros((N, cap, 17, 3), np.float32), kscore=np.zeros((N, cap, 17), np.float32))
    for n, bl in enumerate(bls):
        c = len(bl)
        d["count"][n] = c
        d["score"][n, :c], d["kpt"][n, :c], d["kscore"][n, :c] = bl.get_field("scores"), bl.get_field("keypoints"), bl.get_field("keypoint_logits")
    d["ratios"] = detector._resize_ratios([(im.shape[1], im.shape[0]) for im in images])
    print("detections per image:", d["count"].tolist())
    return d


def _thresholds(d):
    live = np.concatenate([d["score"][n, :d["count"][n]] for n in range(len(d["count"]))])
    thr = _middle(live)
    kthr = _middle(np.concatenate([d["kscore"][n, :d["count"][n]].ravel() for n in range(len(d["count"]))]))
    cand = [int((d["score"][n, :d["count"][n]] > np.float32(thr)).sum()) for n in range(len(d["count"]))]
    return thr, kthr, cand


def _host_composition(net, images, d, thr, kthr, K):
    """MaskRCNN.__call__ (the `detections` fixture) -> the numpy restatement -> Pose2Seg.forward with host keypoints"""
    kp, sc, sl, cnt = ref.handoff(d["score"], d["count"], d["kpt"], d["kscore"], d["ratios"], thr, kthr, K)
    net.forward(images, ref.split(kp, cnt))
    masks, boxes = net.collect()
    N = len(images)
    out = dict(masks=masks, boxes=boxes, count=net.read("count", (N,), np.int32), kp=kp, sc=sc, sl=sl, cnt=cnt, planes=net.read("masks", (N, K, 150, 200), np.uint8))
    out["roi"] = net.read("roi", (int(cnt.sum()), 64, 64, 96)) if cnt.sum() else None
    return out


def _assert_step_equals(pipe, got, want, N, K):
    net = pipe.net
    assert pipe.last["counts"].tolist() == want["cnt"].tolist() and net.read("count", (N,), np.int32).tolist() == want["cnt"].tolist()
    assert np.array_equal(net.read("masks", (N, K, 150, 200), np.uint8), want["planes"])
    if want["roi"] is not None:
        assert same_bits(net.read("roi", want["roi"].shape), want["roi"])
    scores = net.read("scores", (N, K))
    assert same_bits(scores, want["sc"])                                              # the detections' box scores in the live slots, 0 elsewhere
    assert np.array_equal(pipe.source_slots(), want["sl"])
    off = np.concatenate([[0], np.cumsum(want["cnt"])])
    for n in range(N):
        masks, boxes, sc, kp = got[n]
        c = int(want["cnt"][n])
        assert len(masks) == c == len(sc) == len(kp) and boxes.shape == (c, 4)
        assert same_bits(kp, want["kp"][off[n]:off[n + 1]]) and same_bits(sc, want["sc"][n, :c])
        for k in range(c):
            assert np.array_equal(masks[k], want["masks"][n][k]) and same_bits(boxes[k], want["boxes"][n][k]), (n, k)


def test_pipeline_equals_the_host_composition(ffi, detector, detections, p2s_sd):
    from isegmi.pose2seg import KeypointPose2Seg, Pose2Seg, Pose2SegConfig
    images, d = _images(), detections
    thr, kthr, cand = _thresholds(d)
    K = max(cand) - 1                                                                   # the image with the most candidates is cut
    R = sum(min(c, K) for c in cand)
    print("candidates per image:", cand, "K", K, "R", R, "person threshold", thr, "keypoint threshold", kthr)
    assert K >= 1 and 0 < R < int(d["count"].sum()) and any(c > K for c in cand)      # conditions on the inputs, before anything is compared
    net = Pose2Seg(p2s_sd, Pose2SegConfig(), max_batch=3, max_instances=K)
    pipe = KeypointPose2Seg(detector, net, person_threshold=thr, keypoint_threshold=kthr)
    try:
        want = _host_composition(net, images, d, thr, kthr, K)
        assert want["cnt"].sum() == R and set(np.unique(want["kp"][:, :, 2]).tolist()) == {0.0, 2.0}
        got = pipe(images)
        _assert_step_equals(pipe, got, want, 3, K)
        # two steps back to back without a synchronisation between them, the second with fewer persons: nothing of the first survives
        hi = _middle(np.concatenate([d["score"][n, :d["count"][n]][d["score"][n, :d["count"][n]] > np.float32(thr)] for n in range(3)]))
        want_hi = _host_composition(net, images, d, hi, kthr, K)
        assert 0 < want_hi["cnt"].sum() < R
        pipe.forward(images)
        pipe.person_threshold = hi
        pipe.forward(images)
        _assert_step_equals(pipe, pipe.collect(), want_hi, 3, K)
        # nobody passes: zero masks and a zero count
        pipe.person_threshold = 2.0
        got = pipe(images)
        assert pipe.last["R"] == 0 and all(len(g[0]) == 0 and len(g[2]) == 0 and g[3].shape == (0, 17, 3) for g in got)
        assert not net.read("count", (3,), np.int32).any() and not net.read("masks", (3, K, 150, 200), np.uint8).any() and not net.read("scores", (3, K)).any()
        assert (pipe.source_slots() == -1).all()
        pipe.person_threshold = thr                                                     # and the full step again behind the empty one
        _assert_step_equals(pipe, pipe(images), want, 3, K)
    finally:
        pipe.close()
        net.close()


def test_test_from_images_and_the_cli(ffi, detector, detections, p2s_sd, tmp_path):
    from PIL import Image
    from conftest import ROOT
    from isegmi import cli
    from isegmi.coco import rle_encode
    from isegmi.pose2seg import KeypointPose2Seg, Pose2Seg, Pose2SegConfig, test_from_images
    images, d = _images(), detections
    thr, kthr, cand = _thresholds(d)
    K = max(cand) - 1
    assert K >= 1
    net = Pose2Seg(p2s_sd, Pose2SegConfig(), max_batch=3, max_instances=K)
    pipe = KeypointPose2Seg(detector, net, person_threshold=thr, keypoint_threshold=kthr)
    try:
        got = pipe(images)
        expect = [{"image_id": 100 + n, "category_id": 1, "segmentation": rle_encode(m), "score": float(s),
                   "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]}
                  for n, (masks, boxes, sc, _) in enumerate(got) for m, b, s in zip(masks, boxes, sc)]
        kept = ref.handoff(d["score"], d["count"], d["kpt"], d["kscore"], d["ratios"], thr, kthr, K)
        assert len(expect) == int(kept[3].sum()) > 0
        assert [e["score"] for e in expect] == [float(s) for n in range(3) for s in kept[1][n, :kept[3][n]]]   # the box scores, one entry per kept person
        assert test_from_images(pipe, images, [100, 101, 102]) == expect
    finally:
        pipe.close()
        net.close()
    np.savez(tmp_path / "p2s.npz", **p2s_sd)
    np.savez(tmp_path / "kp.npz", **_sd())
    anno = {"images": []}
    for i, im in enumerate(images):
        Image.fromarray(im[:, :, ::-1]).save(tmp_path / ("%d.png" % i))               # the CLI reads BGR like cv2.imread
        anno["images"].append({"id": 100 + i, "file_name": "%d.png" % i, "height": im.shape[0], "width": im.shape[1]})
    (tmp_path / "images.json").write_text(json.dumps(anno))
    out = tmp_path / "segm.json"
    cli.main(["pose2seg_test", "--weights", str(tmp_path / "p2s.npz"), "--anno", str(tmp_path / "images.json"), "--image-root", str(tmp_path),
              "--output", str(out), "--batch-size", "3", "--max-instances", str(K),
              "--keypoint-config", os.path.join(ROOT, "configs", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml"), "--keypoint-weights", str(tmp_path / "kp.npz"),
              "--person-threshold", repr(thr), "--keypoint-threshold", repr(kthr),
              "--keypoint-opts", "INPUT.MIN_SIZE_TEST", str(MIN_SIZE), "INPUT.MAX_SIZE_TEST", str(MAX_SIZE), "MODEL.ROI_HEADS.SCORE_THRESH", str(SCORE_THRESH)])
    assert json.loads(out.read_text()) == expect
