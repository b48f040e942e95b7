"""The deformable-convolution R-CNN models end to end on the HIP engine against tests/maskrcnn_dcn_ref.py: the mdconv Mask R-CNN and the dconv
Faster R-CNN on R-50-FPN, the fused and the unfused form of conv2 on one live engine, a single deformable stage, the shipped yaml through COCODemo and
`cli test_net`, YOLACT++ with the fused form switched on, and the refusals.  Every comparison is bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import maskrcnn_dcn_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


def _assert_dets(out, rd, masks=True):
    for n, (bl, r) in enumerate(zip(out, rd)):
        assert len(bl) == len(r["score"]), (n, len(bl), len(r["score"]))
        assert np.array_equal(bl.get_field("labels"), r["label"].astype(np.int64)), n
        _same(bl.get_field("scores"), r["score"], ("scores", n)); _same(bl.bbox, r["box"], ("boxes", n))
        if masks:
            _same(bl.get_field("mask")[:, 0], r["mask28"], ("mask28", n))


def _has_buffer(model, name):
    from isegmi._ffi import IsegmiError
    try:
        model._buffer_info(name)
        return True
    except IsegmiError as e:
        assert "no such buffer" in str(e), e
        return False


def _assert_stages(model, ref, n, stages=("res3", "res4", "res5")):
    for s in stages:
        _same(model.fetch(s + ".C", n), ref.stage_out[s], s)
    _same(model.fetch("P2", n), ref.feats["P2"], "P2")


COLS = ("backbone.body.layer2.0.col", "backbone.body.layer3.5.col", "backbone.body.layer4.2.col")


def test_mdconv_maskrcnn_batch2_fused_and_unfused_on_one_engine(ffi):
    """Mask R-CNN mdconv R-50 on the 192 x 256 canvas, batch 2: res3 / res4 / res5, P2, boxes, scores, labels and mask28 against the reference with
    dcn_fused 1 from the first forward on -- no .col buffer exists -- then dcn_fused 0 on the same engine (the default: three launches, the .col buffers
    appear), then 1 again."""
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = mr.small()
    assert sum(len(r["score"]) for r in rd) >= 4, "the reference must send detections to the mask head"
    assert float(np.abs(ref.om["backbone.body.layer2.0.conv2"][..., :18]).mean()) > 0.05   # the synthetic offsets are not all ~0
    model = MaskRCNN(mr.state_dict(), x.shape[1], x.shape[2], cfg=mr.config(), max_batch=2)
    try:
        model.set_param("dcn_fused", 1.0)
        out = model(x, hw)
        _same(model.fetch("backbone.body.layer2.0.om", 2), ref.om["backbone.body.layer2.0.conv2"], "offsets / mask logits of res3 block 0")
        _assert_stages(model, ref, 2)
        _assert_dets(out, rd)
        assert not any(_has_buffer(model, c) for c in COLS), "the fused form allocates no column buffer"
        assert _has_buffer(model, "backbone.body.layer2.0.om")
        model.set_param("dcn_fused", 0.0)
        out0 = model(x, hw)
        assert all(_has_buffer(model, c) for c in COLS)
        _assert_stages(model, ref, 2)
        _assert_dets(out0, rd)
        model.set_param("dcn_fused", 1.0)
        _assert_dets(model(x, hw), rd)
        _assert_stages(model, ref, 2)
    finally:
        model.close()


def test_dconv_fasterrcnn_batch1(ffi):
    """Faster R-CNN dconv (DCNv1: 18 offset channels, no mask factor) on the 256 x 352 canvas, batch 1, in both forms."""
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = mr.small(canvas=(256, 352), n=1, modulated=False)
    assert len(rd[0]["score"]) >= 2
    sd = mr.state_dict(modulated=False, mask=False)
    assert sd["backbone.body.layer3.0.conv2.offset.weight"].shape[0] == 18
    model = MaskRCNN(sd, 256, 352, cfg=mr.config(modulated=False, MASK_ON=False), max_batch=1)
    try:
        assert model.box_only
        for fused in (1.0, 0.0):
            model.set_param("dcn_fused", fused)
            out = model(x, hw)
            _assert_stages(model, ref, 1)
            _assert_dets(out, rd, masks=False)
            assert model.fetch("backbone.body.layer3.0.om", 1).shape[-1] == 18
    finally:
        model.close()


def test_single_deformable_stage(ffi):
    """STAGE_WITH_DCN (True, False, False, False): res2 alone (C = 64, the stage without a stride) -- and the other stages stay plain.  Both forms."""
    from isegmi.maskrcnn import MaskRCNN
    stages = (True, False, False, False)
    x, hw, ref, rd = mr.small(n=1, stage_with_dcn=stages)
    model = MaskRCNN(mr.state_dict(stages), x.shape[1], x.shape[2], cfg=mr.config(stages), max_batch=1)
    try:
        for fused in (1.0, 0.0):
            model.set_param("dcn_fused", fused)
            out = model(x, hw)
            _same(model.fetch("res2.C", 1), ref.feats["C2"], "C2")
            _assert_stages(model, ref, 1)
            _assert_dets(out, rd)
        assert _has_buffer(model, "backbone.body.layer1.2.om") and not _has_buffer(model, "backbone.body.layer2.0.om")
        assert not np.array_equal(ref.feats["C2"], mr.small()[2].feats["C2"][:1]), "the deformable stage must matter"
    finally:
        model.close()


def test_fused_launch_is_timed_like_a_convolution(ffi):
    """conv_timing: the fused launch's record carries 2 M 9C Cout FLOPs under the layer's name."""
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = mr.small()
    model = MaskRCNN(mr.state_dict(), x.shape[1], x.shape[2], cfg=mr.config(), max_batch=2)
    try:
        model.upload(x, hw)
        model.set_param("multi_stream", 0.0)
        model.set_param("dcn_fused", 1.0)
        model.forward_device(2); model.sync()
        model.set_param("conv_timing", 1.0)
        buf = C.create_string_buffer(1 << 18)
        ffi.check(ffi.lib().isegmi_engine_conv_report(model._h, buf, 1 << 18))   # drop what the warm-up left
        model.forward_device(2); model.sync()
        ffi.check(ffi.lib().isegmi_engine_conv_report(model._h, buf, 1 << 18))
        rows = {r.split("\t")[0]: float(r.split("\t")[1]) for r in buf.value.decode().strip().split("\n")}
        label = [k for k in rows if k.startswith("backbone.body.layer2.1.conv2 ")]
        assert len(label) == 1 and "deform fused" in label[0] and "K=1152 " in label[0], sorted(rows)[:8]
        M = 2 * 24 * 32   # res3 of the 192 x 256 canvas
        assert rows[label[0]] == pytest.approx(2.0 * M * 9 * 128 * 128 / 1e9, rel=1e-3)
        assert len([k for k in rows if k.startswith("backbone.body.layer2.1.conv2.conv_offset_mask ")]) == 1
    finally:
        model.close()


def test_shipped_mdconv_yaml_through_cocodemo(ffi):
    from isegmi.config import cfg
    from isegmi.maskrcnn import prepare_images
    from isegmi.predictor import COCODemo
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_mask_rcnn_mdconv_R_50_FPN_1x.yaml"))
    image = np.random.default_rng(20261022).integers(0, 256, (192, 256, 3)).astype(np.uint8)
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, max_image_size=256, max_batch=1)
    try:
        assert demo.cfg.STAGE_WITH_DCN == (False, True, True, True) and demo.cfg.WITH_MODULATED_DCN and demo.cfg.depth == 50
        assert demo.state_dict["backbone.body.layer4.2.conv2.offset.weight"].shape == (27, 512, 3, 3)
        p = demo.compute_prediction(image)
        x, hw = prepare_images([image.astype(np.float32)])
        assert x.shape == (1, 192, 256, 3)
        rd = mr.MaskRCNNDcnRef(demo.state_dict).forward(x, hw)[0]
        assert len(p) == len(rd["score"]) > 0
        assert np.array_equal(p.get_field("labels"), rd["label"].astype(np.int64))
        _same(p.get_field("scores"), rd["score"], "scores"); _same(p.bbox, rd["box"], "boxes")
        assert p.get_field("mask").shape == (len(p), 1, 192, 256)
    finally:
        demo.close()


@pytest.mark.parametrize("name", ["e2e_mask_rcnn_mdconv_R_50_FPN_1x.yaml", "e2e_mask_rcnn_dconv_R_50_FPN_1x.yaml", "e2e_faster_rcnn_mdconv_R_50_FPN_1x.yaml",
                                  "e2e_faster_rcnn_dconv_R_50_FPN_1x.yaml"])
def test_cli_test_net_runs_the_shipped_yamls(ffi, tmp_path, name):
    """`python -m isegmi.cli test_net --config-file configs/<dcn yaml> MODEL.WEIGHT random` end to end (at a small test size) writes COCO json."""
    from PIL import Image
    from isegmi import cli
    rng = np.random.default_rng(3)
    src = tmp_path / "in"; src.mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (90 + 10 * i, 120, 3)).astype(np.uint8)).save(src / ("im%d.png" % i))
    out = cli.main(["test_net", "--config-file", os.path.join(ROOT, "configs", name), "--images", str(src), "--output", str(tmp_path / "m.json"),
                    "MODEL.WEIGHT", "random", "INPUT.MIN_SIZE_TEST", "160", "INPUT.MAX_SIZE_TEST", "256"])
    back = json.load(open(tmp_path / "m.json"))
    assert len(back) == len(out) > 0 and {r["image_id"] for r in back} <= {0, 1}
    want = {"image_id", "category_id", "bbox", "score"} | ({"segmentation"} if "mask_rcnn" in name else set())
    assert all(set(r) >= want for r in back)
    assert ("segmentation" in back[0]) == ("mask_rcnn" in name)


def test_plain_r50_and_dcn_engines_coexist(ffi):
    """A plain R-50 model and a deformable one alive in one process, run alternately, leave each other's results unchanged."""
    import fasterrcnn_cases as fc
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = mr.small()
    xp, hwp, refp, rdp = fc.small_reference()
    a = MaskRCNN(mr.state_dict(), x.shape[1], x.shape[2], cfg=mr.config(), max_batch=2)
    b = MaskRCNN(fc.full_state_dict(), xp.shape[1], xp.shape[2], max_batch=2)
    try:
        for rep in range(2):
            _assert_dets(a(x, hw), rd)
            _assert_dets(b(xp, hwp), rdp)
        assert not _has_buffer(b, "backbone.body.layer2.0.om")
    finally:
        a.close(); b.close()


def _arrays(o, path=""):
    if isinstance(o, np.ndarray):
        yield path, o
    elif isinstance(o, dict):
        for k in sorted(o):
            if k != "net":
                yield from _arrays(o[k], path + "/" + str(k))
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            yield from _arrays(v, path + "/" + str(i))


def test_yolact_plus_fused_equals_the_default_three_launches(ffi):
    """yolact_plus_resnet50 on its small test canvas: the default graph is the three launches (the .col buffers exist), dcn_fused = 1 is opt-in and
    gives the same bits everywhere."""
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, YolactConfig, fast_base_transform
    cfg = YolactConfig.plus_resnet50()
    sd = yolact_state_dict(77, depth=cfg.depth, num_priors=9, dcn_layers=cfg.dcn_layers, dcn_interval=cfg.dcn_interval)
    x = fast_base_transform(np.random.default_rng(205).uniform(0, 255, (2, 200, 200, 3)).astype(np.float32))
    net = Yolact(sd, cfg, max_batch=2, input_size=200)
    try:
        net.set_param("step_overlap", 0.0)   # one backbone lane: the same named buffers serve every forward
        base = list(_arrays(net(x)))
        assert _has_buffer(net, "backbone.layers.1.0.col") and _has_buffer(net, "backbone.layers.3.2.col")
        c5 = net.fetch("backbone.layers.3.2.out", 2) if _has_buffer(net, "backbone.layers.3.2.out") else None
        assert len(base) >= 5 and sum(a.size for _, a in base) > 0
        net.set_param("dcn_fused", 1.0)
        fused = list(_arrays(net(x)))
        assert [p for p, _ in fused] == [p for p, _ in base]
        for (p, a), (_, b) in zip(base, fused):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), p
        if c5 is not None:
            _same(net.fetch("backbone.layers.3.2.out", 2), c5, "C5")
        for name in ("P3", "proto"):
            if _has_buffer(net, name):
                assert np.isfinite(net.fetch(name, 2)).all()
    finally:
        net.close()


def test_engine_level_refusals(ffi):
    from isegmi._ffi import IsegmiError
    from isegmi.maskrcnn import MaskRCNN
    with pytest.raises(ValueError, match="STAGE_WITH_DCN.*fp16"):
        MaskRCNN(mr.state_dict(), 128, 160, cfg=mr.config(), max_batch=1, fp16=True)
    with pytest.raises(ValueError, match="conv2.offset.weight.*WITH_MODULATED_DCN"):
        MaskRCNN(mr.state_dict(), 128, 160, cfg=mr.config(modulated=False), max_batch=1)
    with pytest.raises(ValueError, match="conv2.weight.*STAGE_WITH_DCN"):
        from isegmi.weights import maskrcnn_state_dict
        MaskRCNN(maskrcnn_state_dict(1234), 128, 160, cfg=mr.config(), max_batch=1)
    # an offset layer with a channel count that is neither 18 nor 27, set behind the loader's back: the forward names the layer, in both forms
    x, hw, ref, rd = mr.small()
    model = MaskRCNN(mr.state_dict(), x.shape[1], x.shape[2], cfg=mr.config(), max_batch=2)
    try:
        model._set_conv_krsc("backbone.body.layer3.1.conv2.conv_offset_mask", np.zeros((20, 3, 3, 256), np.float32), None, np.zeros(20, np.float32))
        for fused in (1.0, 0.0):
            model.set_param("dcn_fused", fused)
            with pytest.raises(IsegmiError, match=r"backbone\.body\.layer3\.1\.conv2\.conv_offset_mask has 20 output channels"):
                model(x, hw)
    finally:
        model.close()
