"""The YOLOv3-SPP and YOLOv3-tiny engines (csrc/yolov3.cpp, csrc/darknet.cpp, csrc/yolo_pool.hip) against tests/yolo_variants_ref.py, bit for
bit: head tensors, candidate counts and detections on three small canvases, tiny's pad switch flipped on a live engine, the refusals, the command line, and
the default graph next to the new ones.  Weights, inputs and reference forwards are tests/yolo_variants_ref.py's, shared with the CPU tests."""
import dataclasses
import json
import os

import numpy as np
import pytest

import yolo_variants_ref as vr
import yolov3_cases as yc
import yolov3_ref as yr

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cfg(variant, **kw):
    from isegmi.yolov3 import YoloV3Config
    return YoloV3Config.tiny(conf_thresh=vr.ENGINE_CONF, **kw) if variant == "tiny" else YoloV3Config(variant=variant, conf_thresh=vr.ENGINE_CONF, **kw)


@pytest.fixture(scope="module")
def nets(ffi):
    """One engine per (variant, canvas), built on first use, max_batch 2."""
    from isegmi.yolov3 import YoloV3
    made = {}

    def get(variant, H, W):
        if (variant, H, W) not in made:
            made[(variant, H, W)] = YoloV3(vr.engine_weights(variant), H, W, _cfg(variant), max_batch=2)
        return made[(variant, H, W)]
    yield get
    for n in made.values():
        n.close()


def _same_dets(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g["score"]) == len(w["score"])
        assert np.array_equal(g["label"], w["label"]) and np.array_equal(_bits(g["score"]), _bits(w["score"])) and np.array_equal(_bits(g["box"]), _bits(w["box"]))


def _check_forward(net, ref, dets, x):
    got = net(x)
    L = len(ref.feats["heads"])
    heads = net.heads(2)
    assert len(heads) == L == len(net.cfg.strides)
    for s, (g, r) in enumerate(zip(heads, ref.feats["heads"])):
        assert g.shape == r.shape and np.array_equal(_bits(g), _bits(r)), "head %d" % s
    kept, total = net.candidate_counts(2)
    assert total.shape == (2, L) and np.array_equal(total, ref.feats["total"]) and (total >= 1).all()
    assert np.array_equal(kept, [[len(ref.feats["dec"][l][n][1]) for l in range(L)] for n in range(2)])
    _same_dets(got, dets)


@pytest.mark.parametrize("canvas", vr.ENGINE_CANVASES)
@pytest.mark.parametrize("variant", ["spp", "tiny"])
def test_heads_and_detections_bit_exact(nets, variant, canvas):
    """At 32 x 32 the stride-32 map is 1 x 1: every SPP tap but the centre is padding, and tiny's 2 / 1 pool sees a 1 x 1 map."""
    H, W = canvas
    ref, dets = vr.engine_reference(variant, H, W)
    _check_forward(nets(variant, H, W), ref, dets, vr.engine_input(H, W))


def test_spp_block_input_and_output(nets):
    """The SPP block inside the engine: its input is the reference's, its output the reference pool of it (both pad modes)."""
    net = nets("spp", 64, 96)
    x = vr.engine_input(64, 96)
    ref = vr.engine_reference("spp", 64, 96)[0]
    for pad in ("zero", "ignore"):
        net.configure(dataclasses.replace(net.cfg, pool_pad=pad))
        net(x)
        assert np.array_equal(_bits(net.fetch("head.0.t2", 2)), _bits(ref.feats["spp_in"]))
        assert np.array_equal(net.fetch("head.0.spp_cat", 2), vr.spp_concat(ref.feats["spp_in"], pad == "zero"))


@pytest.mark.parametrize("canvas", vr.ENGINE_CANVASES)
def test_tiny_pad_switch_on_a_live_engine(nets, canvas):
    H, W = canvas
    net = nets("tiny", H, W)
    x = vr.engine_input(H, W)
    base = net.cfg
    ign, zero = vr.engine_reference("tiny", H, W), vr.engine_reference("tiny", H, W, zero_pad=True)
    assert all(not np.array_equal(a, b) for a, b in zip(ign[0].feats["heads"], zero[0].feats["heads"]))   # the modes differ on this input
    for pad, (ref, dets) in (("zero", zero), ("ignore", ign), ("zero", zero)):
        net.configure(dataclasses.replace(base, pool_pad=pad))
        _check_forward(net, ref, dets, x)
    net.configure(base)
    _check_forward(net, *ign, x)


def test_default_graph_is_untouched(ffi):
    """A default-variant engine's heads on 64 x 96 against tests/yolov3_ref.py, with the variant parameters set explicitly to their defaults."""
    from isegmi.yolov3 import YoloV3, YoloV3Config
    H, W = 64, 96
    net = YoloV3(yc.engine_weights(), H, W, YoloV3Config(conf_thresh=yc.ENGINE_CONF), max_batch=2)
    try:
        assert net.cfg.variant == "yolov3" and net.cfg.strides == (32, 16, 8)
        ref, dets = yc.engine_reference(H, W)
        got = net(yc.engine_input(H, W))
        for s, (g, r) in enumerate(zip(net.heads(2), ref.feats["heads"])):
            assert np.array_equal(_bits(g), _bits(r)), "head %d" % s
        assert np.array_equal(net.candidate_counts(2)[1], ref.feats["total"])
        _same_dets(got, dets)
        net.set_param("yolo_pool_zero_pad", 1.0)   # no pool in this graph: nothing changes
        _same_dets(net(yc.engine_input(H, W)), dets)
    finally:
        net.close()


def test_refusals(ffi, nets):
    from isegmi.yolov3 import YoloV3, YoloV3Config
    net = nets("tiny", 32, 32)
    n = net.upload(vr.engine_input(32, 32))
    for name, value, back in (("yolo_variant", 3.0, 2.0), ("yolo_variant", -1.0, 2.0), ("yolo_variant", 1.5, 2.0), ("yolo_pool_zero_pad", 2.0, 0.0), ("fp16", 1.0, 0.0),
                              ("graph", 1.0, 0.0)):
        net.set_param(name, value)
        with pytest.raises(ffi.IsegmiError, match=name):
            net.forward_device(n)
        net.set_param(name, back)
    net.forward_device(n)
    net.sync()
    with pytest.raises(ValueError, match="variant"):
        net.configure(dataclasses.replace(net.cfg, variant="spp", anchors=YoloV3Config().anchors, masks=YoloV3Config().masks))
    with pytest.raises(ValueError, match="masks.*two"):   # three levels' worth of anchors for the two-level model
        YoloV3(vr.engine_weights("tiny"), 32, 32, YoloV3Config(variant="tiny"))
    # the same at the C ABI: a tiny engine that was handed yolo_anchor12..17 is refused by name (a fresh engine: a parameter cannot be unset)
    own = YoloV3(vr.engine_weights("tiny"), 32, 32, _cfg("tiny"), max_batch=1)
    try:
        for i in range(12, 18):
            own.set_param("yolo_anchor%d" % i, 10.0)
        own.upload(vr.engine_input(32, 32, 1))
        with pytest.raises(ffi.IsegmiError, match="yolo_anchor12.*two levels"):
            own.forward_device(1)
    finally:
        own.close()


def test_yolo_detect_tiny_end_to_end(ffi, tmp_path):
    """Three synthetic images of different sizes through the command line with --cfg configs/yolov3-tiny.cfg: random weights, and the same through a .weights file."""
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
    wpath = str(tmp_path / "yolov3-tiny.weights")
    save_darknet_weights(vr.engine_weights("tiny"), wpath, variant="tiny")
    common = ["yolo_detect", "--cfg", os.path.join(ROOT, "configs", "yolov3-tiny.cfg"), "--images", str(img_dir), "--img-size", "64", "96", "--conf-thres", "0.05",
              "--batch-size", "2"]
    main(common + ["--weights", "random", "--output", str(tmp_path / "a.json")])
    main(common + ["--weights", wpath, "--output", str(tmp_path / "b.json")])
    main(common + ["--weights", wpath, "--pool-pad", "zero", "--output", str(tmp_path / "c.json")])
    a, b, c = (json.load(open(str(tmp_path / f))) for f in ("a.json", "b.json", "c.json"))
    assert a == b and a != c and len(a) > 0 and {d["image_id"] for d in a} == {0, 1, 2}
    for d in a:
        h, w = sizes[d["image_id"]]
        x, y, bw, bh = d["bbox"]
        assert sorted(d) == ["bbox", "category_id", "image_id", "score"] and d["category_id"] in COCO_CATEGORY_IDS and d["score"] > 0.05
        assert 0 <= x and 0 <= y and bw >= 0 and bh >= 0 and x + bw <= w + 1e-3 and y + bh <= h + 1e-3
