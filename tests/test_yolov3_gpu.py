"""The YOLOv3 engine (csrc/yolov3.cpp, isegmi/yolov3.py) against tests/yolov3_ref.py, bit for bit: raw head tensors, candidate lists and detections on three small
canvases, live parameter changes, the refusals, the command line, and the Yolact Darknet-53 forward through the backbone the two graphs now share.  The seeded
weights, inputs and reference forwards are tests/yolov3_cases.py's, shared with tests/test_yolov3_cpu.py."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

import yolov3_cases as yc
import yolov3_ref as yr

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def nets(ffi):
    """One engine per canvas, built on first use, max_batch 3."""
    from isegmi.yolov3 import YoloV3, YoloV3Config
    made = {}

    def get(H, W):
        if (H, W) not in made:
            made[(H, W)] = YoloV3(yc.engine_weights(), H, W, YoloV3Config(conf_thresh=yc.ENGINE_CONF), max_batch=3)
        return made[(H, W)]
    yield get
    for n in made.values():
        n.close()


def _same_dets(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g["score"]) == len(w["score"])
        assert np.array_equal(g["label"], w["label"]) and np.array_equal(_bits(g["score"]), _bits(w["score"])) and np.array_equal(_bits(g["box"]), _bits(w["box"]))


@pytest.mark.parametrize("canvas", yc.ENGINE_CANVASES)
def test_heads_and_detections_bit_exact(nets, canvas):
    H, W = canvas
    net = nets(H, W)
    ref, dets = yc.engine_reference(H, W)
    got = net(yc.engine_input(H, W))
    for s, (g, r) in enumerate(zip(net.heads(2), ref.feats["heads"])):
        assert g.shape == r.shape == (2, H // yr.STRIDES[s], W // yr.STRIDES[s], 255)
        assert np.array_equal(_bits(g), _bits(r)), "head %d" % s
    kept, total = net.candidate_counts(2)
    assert np.array_equal(total, ref.feats["total"])
    assert np.array_equal(kept, [[len(ref.feats["dec"][l][n][1]) for l in range(3)] for n in range(2)])
    _same_dets(got, dets)


def test_stage_marks(nets):
    net = nets(32, 32)
    net.set_param("timing", 1.0)
    net(yc.engine_input(32, 32))
    names = [n for n, _ in net.timings()]
    net.set_param("timing", 0.0)
    assert [n for n in names if n != "start"] == ["stem", "layer1", "layer2", "layer3", "layer4", "heads", "select", "post"]


def test_parameters_change_and_change_back(nets):
    H, W = 64, 96
    net = nets(H, W)
    x = yc.engine_input(H, W)
    heads, base_total = yc.engine_reference(H, W)[0].feats["heads"], yc.engine_reference(H, W)[0].feats["total"]
    base = net(x)
    _same_dets(base, yc.engine_reference(H, W)[1])
    cfg = net.cfg
    for change in (dict(multi_label=False), dict(conf_thresh=0.08), dict(nms_thresh=0.6), dict(pre_nms_top_n=50), dict(min_wh=24.0),
                   dict(detections_per_img=7), dict(nms_plus_one=1, nms_ge=1)):
        c = dataclasses.replace(cfg, **change)
        net.configure(c)
        flags = (0 if c.nms_plus_one else 2) | (1 if c.nms_ge else 0)
        _, total, want = yr.tail(heads, nms_thr=c.nms_thresh, det_per_img=c.detections_per_img, cap=c.det_cap, nms_flags=flags, top_n=c.pre_nms_top_n,
                                 thr=c.conf_thresh, multi_label=c.multi_label, min_wh=c.min_wh, canvas_w=W, canvas_h=H)
        got = net(x)
        _same_dets(got, [dict(box=d[0], score=d[1], label=d[2]) for d in want])
        assert np.array_equal(net.candidate_counts(2)[1], total)
        # the change is visible: in the detections, or (a threshold under the 100 best scores) in the candidate counts
        assert not np.array_equal(total, base_total) or any(len(g["score"]) != len(b["score"]) or not np.array_equal(g["box"], b["box"]) for g, b in zip(got, base)), change
        net.configure(cfg)
        _same_dets(net(x), base)


def test_refusals(ffi, nets):
    from isegmi.yolov3 import YoloV3, YoloV3Config
    net = nets(32, 32)
    x = yc.engine_input(32, 32)
    n = net.upload(x)
    for name, value, back in (("fp16", 1.0, 0.0), ("graph", 1.0, 0.0), ("yolo_pre_nms_top_n", 1025.0, 1024.0), ("yolo_conf_thresh", -1.0, yc.ENGINE_CONF)):
        net.set_param(name, value)
        with pytest.raises(ffi.IsegmiError, match=name):
            net.forward_device(n)
        net.set_param(name, back)
    net.forward_device(n)
    net.sync()
    with pytest.raises(ffi.IsegmiError, match="not a yolact engine"):
        ffi.check(ffi.lib().isegmi_yolact_forward(net._h, net.input_buffer().ptr, 1))
    h = C.c_void_p()
    with pytest.raises(ffi.IsegmiError, match="5 yolov3"):
        ffi.check(ffi.lib().isegmi_engine_create(6, 1, 32, 32, C.byref(h)))
    with pytest.raises(ffi.IsegmiError, match="multiples of 32"):
        ffi.check(ffi.lib().isegmi_engine_create(5, 1, 48, 32, C.byref(h)))
    with pytest.raises(RuntimeError, match="box detector"):
        net.rle_device()
    with pytest.raises(ValueError, match="fp16"):
        YoloV3(yc.engine_weights(), 32, 32, YoloV3Config(), fp16=True)


def test_yolo_detect_end_to_end(ffi, tmp_path):
    """Three synthetic images of different sizes through the command line, with random weights and with the same weights read from a .weights file."""
    from PIL import Image
    from isegmi.cli import main
    from isegmi.coco import COCO_CATEGORY_IDS
    from isegmi.weights import save_darknet_weights
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    rng = np.random.default_rng(3)
    sizes = [(40, 70), (90, 50), (64, 64)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(img_dir / ("im%d.png" % i)))
    wpath = str(tmp_path / "yolov3.weights")
    save_darknet_weights(yc.engine_weights(), wpath)
    common = ["yolo_detect", "--cfg", os.path.join(ROOT, "configs", "yolov3.cfg"), "--images", str(img_dir), "--img-size", "64", "96", "--conf-thres", "0.05",
              "--batch-size", "2"]
    main(common + ["--weights", "random", "--output", str(tmp_path / "a.json")])
    main(common + ["--weights", wpath, "--output", str(tmp_path / "b.json")])
    a, b = json.load(open(str(tmp_path / "a.json"))), json.load(open(str(tmp_path / "b.json")))
    assert a == b and len(a) > 0 and {d["image_id"] for d in a} == {0, 1, 2}
    for d in a:
        h, w = sizes[d["image_id"]]
        x, y, bw, bh = d["bbox"]
        assert sorted(d) == ["bbox", "category_id", "image_id", "score"] and d["category_id"] in COCO_CATEGORY_IDS and d["score"] > 0.05
        assert 0 <= x and 0 <= y and bw >= 0 and bh >= 0 and x + bw <= w + 1e-3 and y + bh <= h + 1e-3


def test_yolact_darknet_forward_is_unchanged(ffi):
    """yolact_darknet53_config through the backbone now shared with YOLOv3: bit-equal to YolactRef, as before the move."""
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, YolactConfig, darknet_base_transform
    from oracle.yolact_ref import YolactRef
    sd = yolact_state_dict(31, backbone="darknet53")
    size = 136
    x = darknet_base_transform(np.random.default_rng(8).uniform(0, 255, (1, size, size, 3)).astype(F32))
    net = Yolact(sd, YolactConfig.darknet53(), max_batch=1, input_size=size)
    ref = YolactRef(sd, max_size=550)
    out = net(x)
    r = ref.forward(x)[0]
    for name, eng in (("C3", "backbone.layers.2.8.out"), ("P3", "P3"), ("P7", "P7"), ("proto", "proto")):
        assert np.array_equal(net.fetch(eng, 1).reshape(ref.feats[name].shape), ref.feats[name]), name
    d = out[0]["detection"]
    assert len(r["score"]) > 0 and d is not None
    for a, b in (("prior", "prior"), ("class", "cls"), ("score", "score"), ("box", "box"), ("mask", "mask")):
        assert np.array_equal(d[a], r[b]), a
    net.close()
