"""Keypoint R-CNN on the HIP engine (MODEL.KEYPOINT_ON) on the 128 x 160 canvas: the keypoint head stage by stage on the engine's own
intermediates against tests/keypoint_ref.py and the oracle, the box path against a box-only engine on the same trunk, determinism, graph replay, the
keypoint record block, COCODemo / inference() and the refusals.  Every comparison is bit for bit."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import fasterrcnn_cases as fc
import keypoint_cases as kc
import keypoint_ref as kr
from conv_ref import same_bits
from oracle import ora

pytestmark = pytest.mark.gpu

FX = "roi_heads.keypoint.feature_extractor.conv_fcn"
HEAD_BUFS = ("det.kpt", "det.kscore")


SCORE_THRESH = 0.012   # the seeded two-class predictor keeps its 81-class background bias: at upstream's 0.05 an image has one or two detections


def _cfg(**kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return dataclasses.replace(MaskRCNNConfig(), **{**dict(MASK_ON=False, NUM_CLASSES=2, KEYPOINT_ON=True, ROI_SCORE_THRESH=SCORE_THRESH), **kw})


@functools.lru_cache(maxsize=None)
def _sd():
    from isegmi.weights import keypointrcnn_state_dict
    return keypointrcnn_state_dict(1234)


@functools.lru_cache(maxsize=None)
def _batch():
    """Three images on the 128 x 160 canvas."""
    from isegmi.maskrcnn import prepare_images
    rng = np.random.default_rng(20261019)
    x, hw = prepare_images([rng.uniform(0, 255, s).astype(np.float32) for s in ((100, 130, 3), (120, 150, 3), (128, 101, 3))])
    assert x.shape[1:3] == (128, 160)
    x.setflags(write=False)
    return x, hw


@pytest.fixture(scope="module")
def engine(ffi):
    from isegmi.maskrcnn import MaskRCNN
    m = MaskRCNN(_sd(), 128, 160, cfg=_cfg(), max_batch=3)
    yield m
    m.close()


def _run(m, n, forwards=1):
    x, hw = _batch()
    m.upload(x[:n], hw[:n])
    for _ in range(forwards):
        m.forward_device(n)
    m.sync()
    out = {k: m.fetch(k, n).copy() for k in fc.DET_KEYS + HEAD_BUFS}
    return out


def _same(a, b, what):
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("bs", [1, 2])
def test_keypoint_head_stage_by_stage(engine, bs):
    """Fetched det.box / det.count and P2..P5 go in; every buffer of the head is compared against the restatement fed with the engine's own previous buffer:
    kp.roi_feat (every live slot); kp.fcn1..8 on a band of four rows of one detection per layer -- rows 0..3, 5..8 or 10..13 (a band needs one input row
    more on each side that exists), band and slot rotated over the layers and the batch sizes, the first and the last live slot of every image among them --
    and one WHOLE layer of the last live slot (fcn1 at bs 1, fcn8 at bs 2): the CPU oracle takes a second per detection and layer at 512 channels;
    kp.lowres68 on eight slots per image; kp.heat, det.kpt and det.kscore on every live slot (empty slots zero)."""
    from isegmi.maskrcnn import pack_keypoint_deconv
    from isegmi.weights import to_krsc
    m, sd = engine, _sd()
    got = _run(m, bs)
    cap = 100
    cnt = got["det.count"]
    print("detections per image:", cnt.tolist())
    assert (cnt > 5).all() and got["det.kpt"].shape == (bs, cap, 17, 3) and got["det.kscore"].shape == (bs, cap, 17)
    P = [m.fetch(k, bs) for k in ("P2", "P3", "P4", "P5")]
    live = [n * cap + c for n in range(bs) for c in range(int(cnt[n]))]
    ends = [s_ for n in range(bs) for s_ in (n * cap, n * cap + int(cnt[n]) - 1)]   # first and last live slot of every image
    roi = m.fetch("kp.roi_feat")
    for n in range(bs):
        D = int(cnt[n])
        assert same_bits(roi[n * cap:n * cap + D], kr.roi_features(P, got["det.box"][n, :D], n)), n
    BANDS = ((0, 5, 0, 4), (4, 10, 5, 9), (9, 14, 10, 14))   # input rows [a, b) give output rows [c, d) exactly
    whole = 1 if bs == 1 else 8
    prev = roi
    for i in range(1, 9):
        cur = m.fetch("kp.fcn%d" % i)
        assert cur.shape == (bs * cap, 14, 14, 512)
        slot = ends[(i + bs) % len(ends)] if i % 2 else live[(i * 37 + bs * 11) % len(live)]
        ia, ib, oa, ob = BANDS[(i + bs) % 3]
        w, b = to_krsc(sd["%s%d.weight" % (FX, i)]), sd["%s%d.bias" % (FX, i)]
        band = ora.conv2d(prev[slot:slot + 1, ia:ib], w, 1, 1, None, b, None, 1)[0]
        assert same_bits(cur[slot, oa:ob], band[oa - ia:ob - ia]), (i, slot, oa)
        if i == whole:
            last = ends[-1]
            assert same_bits(cur[last], ora.conv2d(prev[last:last + 1], w, 1, 1, None, b, None, 1)[0]), ("whole layer", i)
        assert cur[slot].min() == 0 and cur[slot].max() > 0                       # ReLU, and alive
        prev = cur
    low = m.fetch("kp.lowres68")
    assert low.shape == (bs * cap, 14, 14, 68)
    w3, b4 = pack_keypoint_deconv(sd["roi_heads.keypoint.predictor.kps_score_lowres.weight"], sd["roi_heads.keypoint.predictor.kps_score_lowres.bias"])
    some = sorted({n * cap + (int(cnt[n]) - 1) * j // 7 for n in range(bs) for j in range(8)})
    assert same_bits(low[some], ora.conv2d(prev[some], w3, 1, 1, None, b4, None, 0))
    heat = m.fetch("kp.heat")
    assert heat.shape == (bs * cap, 56, 56, 17)
    assert same_bits(heat[live], kr.heatmap(low[live], 17))
    want_kpt, want_ks = kr.decode(heat[:bs * cap], got["det.box"], cnt)
    assert same_bits(got["det.kpt"], want_kpt) and same_bits(got["det.kscore"], want_ks)
    assert len(np.unique(got["det.kpt"][0, :int(cnt[0]), :, :2].reshape(-1, 2), axis=0)) > 17   # keypoints differ between detections and channels


def test_box_path_equals_a_box_only_engine_on_the_same_trunk(ffi, engine):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw = _batch()
    box = MaskRCNN(maskrcnn_state_dict(1234, mask=False, num_classes=2), 128, 160, cfg=_cfg(KEYPOINT_ON=False), max_batch=3)
    try:
        assert box.box_only and not box.keypoint_on and engine.box_only and engine.keypoint_on
        mem_box, mem_kp = box.reserve(), engine.reserve()
        assert mem_box[0] < mem_kp[0] and mem_box[1] < mem_kp[1]
        box.upload(x[:2], hw[:2]); box.forward_device(2); box.sync()
        want = fc.fetch_dets(box, 2)
        _run(engine, 2)
        fc.assert_same_dets(fc.fetch_dets(engine, 2), want, "keypoint engine vs box-only engine")
        assert int(want["det.count"].sum()) > 2
        for name in ("kp.roi_feat", "kp.heat", "det.kpt"):                         # the box-only engine has none of the head's buffers ...
            with pytest.raises(ffi.IsegmiError, match="no such buffer"):
                box.fetch(name)
        for name in ("det.mask28", "mask.roi_feat", "mask.deconv", "det.masks"):   # ... and the keypoint engine none of the mask head's, reserve() included
            with pytest.raises(ffi.IsegmiError, match="no such buffer"):
                engine.fetch(name)
        assert engine.coco_record_bytes(2) == (kc.block_bytes(2, 100), kc.block_bytes(2, 100)) and box.coco_record_bytes(2)[0] == fc.box_block_bytes(2, 100)
    finally:
        box.close()


def test_forwards_are_deterministic_and_batch_independent(engine):
    a = _run(engine, 2, forwards=2)      # two forwards back to back, no synchronisation between them
    b = _run(engine, 2)
    _same(a, b, "second run of the batch")
    c = _run(engine, 1)                  # then another batch size: image 0 alone on the same canvas
    for k in a:
        assert same_bits(a[k][:1], c[k]), k
    d = _run(engine, 3)
    for k in a:
        assert same_bits(a[k], d[k][:2]), k


def test_graph_replay_equals_eager(ffi, engine):
    import ctypes as C
    want = {n: _run(engine, n) for n in (2, 1)}
    engine.set_param("graph", 1.0)
    try:
        for rep in range(3):             # eager warm-up or capture, then replays
            for n in (2, 1):
                _same(_run(engine, n), want[n], ("graph", rep, n))
        cap, rep_, fail = C.c_int64(), C.c_int64(), C.c_int64()
        ffi.check(ffi.lib().isegmi_engine_graph_stats(engine._h, C.byref(cap), C.byref(rep_), C.byref(fail)))
        assert cap.value >= 2 and rep_.value >= 2 and fail.value == 0
    finally:
        engine.set_param("graph", 0.0)
    _same(_run(engine, 2), want[2], "eager again")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_keypoint_records_against_numpy(ffi, engine, n):
    """isegmi_engine_pack_keypoint_records on its own: n images in a block of three slots, ratios != 1 -- every byte of the block against numpy (sections,
    the zero padding between them, the empty slots), and nothing written past it."""
    from isegmi.dist import unpack_coco_records
    got = _run(engine, n)
    sizes = [(333, 517), (160, 128), (77, 401)][:n]
    engine.set_output_sizes(sizes)
    total = kc.block_bytes(3, 100)
    dev = ffi.DeviceBuffer.from_numpy(np.full(total + 64, 0xa5, np.uint8))
    assert engine.pack_keypoint_records(dev, 3) == total == engine.coco_record_bytes(3)[0]
    engine.sync()
    raw = dev.numpy()
    assert (raw[total:] == 0xa5).all()
    _, hw = _batch()
    ratios = np.array([[w / hw[i][1], h / hw[i][0]] for i, (w, h) in enumerate(sizes)]).astype(np.float32)
    assert (ratios != 1).all()
    want = kr.pack_records(got["det.box"], got["det.count"], got["det.score"], got["det.label"], got["det.kpt"], got["det.kscore"], ratios, 3)
    assert np.array_equal(raw[:total], want)
    rec = unpack_coco_records(raw, 3, 100, 2, box_only=True, keypoints=17)
    D = int(got["det.count"][0])
    assert rec["count"].tolist() == got["det.count"].tolist() + [0] * (3 - n) and D > 0
    assert np.array_equal(rec["kpt"][0, :D, :, 0], got["det.kpt"][0, :D, :, 0] * ratios[0, 0]) and (rec["kpt"][0, :D, :, 2] == 1).all()
    assert not rec["kpt"][0, D:].any() and not rec["kscore"][0, D:].any() and not rec["kpt"][n:].any() and not rec["box"][n:].any()
    small = ffi.DeviceBuffer((total - 8,), np.uint8)
    with pytest.raises(ffi.IsegmiError, match="too small"):
        engine.pack_keypoint_records(small, 3)


def _demo_images():
    from conftest import smooth_field
    rng = np.random.default_rng(41)
    return [rng.integers(0, 256, (150, 200, 3)).astype(np.uint8), np.ascontiguousarray(smooth_field(7, 200, 150), np.uint8),
            rng.integers(0, 256, (150, 200, 3)).astype(np.uint8)]


def test_cocodemo_and_inference_write_keypoint_results(ffi, tmp_path):
    """COCODemo with the keypoint yaml on three small images in two canvases, bs = 2: inference() -- the keypoint block through the two-slot download, and
    again through the RCCL all-gather of a world of one -- equals the entries built from the buffers compute_prediction fetched."""
    import json
    from conftest import ROOT
    from isegmi.coco import label_categories, maskrcnn_results
    from isegmi.config import cfg
    from isegmi.predictor import COCODemo, inference
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml"))
    c.merge_from_list(["MODEL.ROI_HEADS.SCORE_THRESH", SCORE_THRESH])
    images = _demo_images()
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, state_dict=_sd(), max_image_size=320, max_batch=2)
    try:
        model = demo.engine()
        assert demo.box_only and model.keypoint_on and demo.cfg.KEYPOINT_ON and demo.CATEGORIES == ("__background", "class 1")
        direct = []
        for i, im in enumerate(images):
            p = demo.compute_prediction(im)
            assert sorted(p.fields()) == ["keypoint_logits", "keypoints", "labels", "scores"] and p.size == (im.shape[1], im.shape[0])
            kp = p.get_field("keypoints")
            assert kp.shape == (len(p), 17, 3) and p.get_field("keypoint_logits").shape == (len(p), 17) and kp.dtype == np.float32
            assert (kp[:, :, 2] == 1).all() and (kp[:, :, 0] >= p.bbox[:, None, 0]).all() and (kp[:, :, 0] <= p.bbox[:, None, 2] + 1).all()
            direct += maskrcnn_results(10 + i, p.bbox, p.get_field("scores"), p.get_field("labels"), categories=label_categories(2), keypoints=kp)
        print("demo detections:", len(direct))
        assert len(direct) > 10
        st = {}
        res = inference(demo, images, image_ids=[10, 11, 12], batch_size=2, stats=st)
        assert st["steps"] == 2 and st["images"] == 3
        gathered = inference(demo, images, image_ids=[10, 11, 12], batch_size=2, force_gather=True)
        assert res == direct and gathered == direct
        path = tmp_path / "keypoints.json"
        path.write_text(json.dumps(res))
        back = json.loads(path.read_text())
        assert all(d["category_id"] == 1 and len(d["keypoints"]) == 51 and len(d["bbox"]) == 4 and "segmentation" not in d for d in back)
        out = demo.run_on_opencv_image(images[0])
        assert out.shape == images[0].shape and out.dtype == np.uint8 and (out != images[0]).any()
    finally:
        demo.close()


def test_zero_detections_give_no_entries_and_a_zero_count(ffi):
    from isegmi.pipeline import RecordPipeline
    from isegmi.predictor import COCODemo, inference
    from isegmi.transforms import maskrcnn_resize_u8
    sd = dict(_sd())
    sd["roi_heads.box.predictor.cls_score.bias"] = sd["roi_heads.box.predictor.cls_score.bias"].copy()
    sd["roi_heads.box.predictor.cls_score.bias"][0] += 50.0
    images = _demo_images()
    demo = COCODemo(_cfg(), min_image_size=192, confidence_threshold=0.0, state_dict=sd, max_image_size=320, max_batch=2)
    try:
        assert inference(demo, images, batch_size=2) == []
        model = demo.engine()
        n = model.upload_u8([maskrcnn_resize_u8(images[0], 192, 320)])
        model.forward_device(n)
        model.set_output_sizes([(200, 150)])
        with RecordPipeline(model, 2) as pipe:
            assert pipe.box_only and pipe.keypoints == 17 and pipe.nbytes == kc.block_bytes(2, 100)
            pipe.submit("step")
            (meta, (rec,)), = pipe.flush()
            assert meta == "step" and not rec["count"].any() and not rec["kpt"].any() and not rec["kscore"].any() and rec["overflow"] is None
    finally:
        demo.close()


def test_engine_refusals(ffi):
    """The engine's own refusals, each by name: keypoint_on with mask_on, fp16, the C4 body and GroupNorm weights; a keypoint engine without the head's layers;
    pack_keypoint_records on an engine without the head."""
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw = _batch()
    m = MaskRCNN(maskrcnn_state_dict(1234, mask=False, num_classes=2), 128, 160, cfg=_cfg(KEYPOINT_ON=False), max_batch=1)
    try:
        m.upload(x[:1], hw[:1]); m.forward_device(1); m.sync()
        dev = ffi.DeviceBuffer((kc.block_bytes(1, 100),), np.uint8)
        with pytest.raises(ffi.IsegmiError, match="keypoint_on 0"):
            m.pack_keypoint_records(dev, 1)
        m.set_param("keypoint_on", 1.0)
        with pytest.raises(ffi.IsegmiError, match="kps_score_lowres"):             # no head weights were loaded
            m.forward_device(1)
        m.sync()
        for name, value, match in (("mask_on", 1.0, "mask_on 1"), ("fp16", 1.0, "fp16"), ("arch_c4", 1.0, "arch_c4"), ("num_keypoints", 33.0, "num_keypoints")):
            m.set_param(name, value)
            with pytest.raises(ffi.IsegmiError, match="keypoint_on 1.*" + match if name != "num_keypoints" else match):
                m.forward_device(1)
            m.sync()
            m.set_param(name, {"num_keypoints": 17.0}.get(name, 0.0))
        m._set_tensor("backbone.body.stem.conv1.gn.weight", np.ones(64, np.float32))
        with pytest.raises(ffi.IsegmiError, match="keypoint_on 1.*GroupNorm"):
            m.forward_device(1)
        m.sync()
    finally:
        m.close()
