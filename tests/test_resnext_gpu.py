"""The ResNeXt models end to end on the HIP engine against references composed from the oracle ops (tests/resnext_ref.py): Mask R-CNN,
Faster R-CNN and RetinaNet on X-50-32x8d -- the four group widths of X-101-32x8d at a fraction of the weights -- in every launch form, and the shipped
X-101 yaml through COCODemo.  Every comparison is bit for bit."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import resnext_ref as xr

pytestmark = pytest.mark.gpu


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


def _graph_stats(model):
    from isegmi import _ffi
    cap, rep, fail = C.c_int64(), C.c_int64(), C.c_int64()
    _ffi.check(_ffi.lib().isegmi_engine_graph_stats(model._h, C.byref(cap), C.byref(rep), C.byref(fail)))
    return cap.value, rep.value, fail.value


def test_maskrcnn_x50_batch2_bit_exact(ffi):
    """C2, P2-P6, proposals, detections, 28 x 28 masks and pasted masks; then the same forward as a hipGraph replay."""
    from isegmi.maskrcnn import MaskRCNN
    from oracle.maskrcnn_ref import MaskRCNNRef
    x, hw, ref, rd = xr.small()
    assert sum(len(r["score"]) for r in rd) >= 8, "the reference must send detections to the mask head"
    model = MaskRCNN(xr.state_dict(), x.shape[1], x.shape[2], cfg=xr.config(), max_batch=2)
    try:
        out = model(x, hw)
        _same(model.fetch("res2.C", 2), ref.feats["C2"], "C2")
        for name in ("P2", "P3", "P4", "P5", "P6"):
            _same(model.fetch(name, 2), ref.feats[name], name)
        pc = model.fetch("proposal_count", 2); pr = model.fetch("proposals", 2); ps = model.fetch("proposal_scores", 2)
        for n in range(2):
            assert pc[n] == len(rd[n]["proposals"])
            _same(ps[n, : pc[n]], rd[n]["proposal_scores"], "proposal scores"); _same(pr[n, : pc[n]], rd[n]["proposals"], "proposals")
        _assert_dets(out, rd)
        assert sum(len(bl) for bl in out) >= 8
        model.paste_device(x.shape[1], x.shape[2]); model.sync()
        masks = model.fetch("det.masks", 2)
        for n in range(2):
            rm, _ = MaskRCNNRef.paste(rd[n], x.shape[1], x.shape[2])
            assert np.array_equal(masks[n, : len(rm)], rm), n
        # hipGraph: eager once more (warm), capture, replay -- all equal to the eager result
        model.set_param("graph", 1.0)
        for rep in range(3):
            _assert_dets(model(x, hw), rd)
        cap, reps, fail = _graph_stats(model)
        assert fail == 0 and cap >= 1 and reps >= 1, (cap, reps, fail)
        _same(model.fetch("P2", 2), ref.feats["P2"], "P2 after the replay")
    finally:
        model.close()


def test_maskrcnn_x50_stride_in_1x1_true(ffi):
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = xr.small(stride_in_1x1=True, n=1)
    model = MaskRCNN(xr.state_dict(), x.shape[1], x.shape[2], cfg=xr.config(STRIDE_IN_1X1=True), max_batch=1)
    try:
        out = model(x, hw)
        _same(model.fetch("P2", 1), ref.feats["P2"], "P2")
        _assert_dets(out, rd)
        assert len(out[0]) >= 8
        assert not np.array_equal(ref.feats["P2"], xr.small()[2].feats["P2"][:1]), "the stride placement must matter"
    finally:
        model.close()


def test_maskrcnn_x50_split_k_leaves_the_grouped_layers_unsplit(ffi):
    """conv_split_k on: the dense bottleneck layers take the split-K evaluation by the shape rule (the reference mirrors it), the grouped ones never do."""
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = xr.small(conv_split_k=1, n=1)
    model = MaskRCNN(xr.state_dict(), x.shape[1], x.shape[2], cfg=xr.config(CONV_SPLIT_K=1), max_batch=1)
    try:
        out = model(x, hw)
        for name in ("P2", "P5", "P6"):
            _same(model.fetch(name, 1), ref.feats[name], name)
        _assert_dets(out, rd)
        assert not np.array_equal(ref.feats["P5"], xr.small()[2].feats["P5"][:1]), "the mode must change low bits of the dense layers"
    finally:
        model.close()


def test_fasterrcnn_x50_box_only(ffi):
    """MASK_ON False on the ResNeXt body: the mask reference's boxes, scores and labels; the box-only record block packs."""
    import fasterrcnn_cases as fc
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw, ref, rd = xr.small()
    sd = maskrcnn_state_dict(xr.SEED, 50, mask=False, groups=xr.GROUPS, width_per_group=xr.WIDTH)
    model = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=xr.config(MASK_ON=False), max_batch=2)
    try:
        assert model.box_only
        out = model(x, hw)
        _assert_dets(out, rd, masks=False)
        assert all(not bl.has_field("mask") for bl in out)
        from isegmi.dist import unpack_coco_records
        model.set_output_sizes([(int(hw[n][1]), int(hw[n][0])) for n in range(2)])   # (w, h): ratio 1
        dev = ffi.DeviceBuffer.from_numpy(np.full(fc.box_block_bytes(2, 100) + 64, 0xa5, np.uint8))
        assert model.pack_box_records(dev, 2) == fc.box_block_bytes(2, 100)
        model.sync()
        raw = dev.numpy()
        assert (raw[fc.box_block_bytes(2, 100):] == 0xa5).all()
        rec = unpack_coco_records(raw, 2, 100, 2, box_only=True)
        for n in range(2):
            D = len(rd[n]["score"])
            assert rec["count"][n] == D
            _same(rec["box"][n, :D], rd[n]["box"], "record boxes"); _same(rec["score"][n, :D], rd[n]["score"], "record scores")
    finally:
        model.close()


def test_retinanet_x50(ffi):
    import retinanet_common as rc
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    x, hw, ref, dets = xr.retina_small()
    cfg = RetinaNetConfig(DETECTIONS_CAP=128, NUM_GROUPS=xr.GROUPS, WIDTH_PER_GROUP=xr.WIDTH, STRIDE_IN_1X1=False)
    m = RetinaNet(xr.retina_state_dict(), 256, 352, cfg, max_batch=2)
    try:
        preds = m(x, hw)
        rc.assert_forward_equal(m, ref, 2)
        rc.assert_dets_equal(preds, dets)
        assert sum(len(p) for p in preds) > 20
    finally:
        m.close()


def test_shipped_x101_yaml_through_cocodemo(ffi):
    """configs/e2e_mask_rcnn_X_101_32x8d_FPN_1x.yaml with random weights, one 192 x 256 image: the one test that carries the full 32x8d-101 weights."""
    from conftest import ROOT
    from isegmi.config import cfg
    from isegmi.maskrcnn import prepare_images
    from isegmi.predictor import COCODemo
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_mask_rcnn_X_101_32x8d_FPN_1x.yaml"))
    image = np.random.default_rng(20261020).integers(0, 256, (192, 256, 3)).astype(np.uint8)
    demo = COCODemo(c, min_image_size=192, confidence_threshold=0.0, max_image_size=256, max_batch=1)
    try:
        assert demo.cfg.NUM_GROUPS == 32 and demo.cfg.WIDTH_PER_GROUP == 8 and demo.cfg.depth == 101 and not demo.cfg.STRIDE_IN_1X1
        assert demo.state_dict["backbone.body.layer3.22.conv2.weight"].shape == (1024, 32, 3, 3)
        p = demo.compute_prediction(image)
        x, hw = prepare_images([image.astype(np.float32)])
        assert x.shape == (1, 192, 256, 3)
        rd = xr.ResNeXtRef(demo.state_dict, depth=101).forward(x, hw)[0]
        assert len(p) == len(rd["score"]) > 0
        assert np.array_equal(p.get_field("labels"), rd["label"].astype(np.int64))
        _same(p.get_field("scores"), rd["score"], "scores"); _same(p.bbox, rd["box"], "boxes")
        assert p.get_field("mask").shape == (len(p), 1, 192, 256)
    finally:
        demo.close()


def test_r50_and_x50_engines_coexist(ffi):
    """An R-50 FrozenBN model and an X-50 model alive in one process, run alternately, leave each other's results unchanged."""
    import fasterrcnn_cases as fc
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = xr.small()
    xr50, hwr, refr, rdr = fc.small_reference()
    a = MaskRCNN(xr.state_dict(), x.shape[1], x.shape[2], cfg=xr.config(), max_batch=2)
    b = MaskRCNN(fc.full_state_dict(), xr50.shape[1], xr50.shape[2], max_batch=2)
    try:
        for rep in range(2):
            _assert_dets(a(x, hw), rd)
            _assert_dets(b(xr50, hwr), rdr)
    finally:
        a.close(); b.close()


def test_engine_refuses_grouped_layers_where_they_are_not_built(ffi):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    with pytest.raises(ValueError, match="NUM_GROUPS.*fp16"):
        MaskRCNN(xr.state_dict(), 128, 160, cfg=xr.config(), max_batch=1, fp16=True)
    with pytest.raises(ValueError, match="conv2.weight"):          # a ResNeXt dict under a ResNet config
        MaskRCNN(xr.state_dict(), 128, 160, cfg=MaskRCNNConfig(), max_batch=1)
    with pytest.raises(ValueError, match="conv2.weight"):          # and the other way round
        MaskRCNN(maskrcnn_state_dict(1234), 128, 160, cfg=xr.config(), max_batch=1)


def test_timing_record_counts_the_grouped_flops(ffi):
    """conv_timing: a grouped layer's record carries 2 M Cout 9 (Cin / groups) FLOPs -- a 32nd of the dense count -- and says `groups=32`."""
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = xr.small()
    model = MaskRCNN(xr.state_dict(), x.shape[1], x.shape[2], cfg=xr.config(), max_batch=2)
    try:
        model.upload(x, hw)
        model.set_param("multi_stream", 0.0)
        model.forward_device(2); model.sync()
        model.set_param("conv_timing", 1.0)
        buf = C.create_string_buffer(1 << 18)
        ffi.check(ffi.lib().isegmi_engine_conv_report(model._h, buf, 1 << 18))   # drop what the warm-up left
        model.forward_device(2); model.sync()
        ffi.check(ffi.lib().isegmi_engine_conv_report(model._h, buf, 1 << 18))
        rows = {r.split("\t")[0]: float(r.split("\t")[1]) for r in buf.value.decode().strip().split("\n")}
        label = [k for k in rows if k.startswith("backbone.body.layer1.1.conv2 ")]
        assert len(label) == 1 and "groups=32" in label[0] and "K=72 " in label[0], sorted(rows)[:8]
        M = 2 * 64 * 88   # res2 of the 256 x 352 canvas
        assert rows[label[0]] == pytest.approx(2.0 * M * 256 * 9 * 8 / 1e9, rel=1e-3)
        entry = [k for k in rows if k.startswith("backbone.body.layer2.0.conv2 ")]
        assert len(entry) == 1 and "3x3/2" in entry[0] and "groups=32" in entry[0]
    finally:
        model.close()


def test_engine_entry_point_refuses_by_name(ffi):
    """isegmi_engine_set_conv_grouped on an fp16 engine, a C4 body, a Yolact engine, and with weights the kernel does not take."""
    w = np.zeros((64, 3, 3, 8), np.float32)
    wp = w.ctypes.data_as(C.c_void_p)
    L = ffi.lib()

    def engine(kind, **params):
        h = C.c_void_p()
        ffi.check(L.isegmi_engine_create(kind, 1, 64, 64, C.byref(h)))
        for k, v in params.items():
            ffi.check(L.isegmi_engine_set_param(h, k.encode(), C.c_float(v)))
        return h

    for kind, params, word in ((2, dict(fp16=1.0), b"fp16"), (2, dict(arch_c4=1.0), b"C4"), (1, {}, b"Mask R-CNN and RetinaNet")):
        h = engine(kind, **params)
        try:
            assert L.isegmi_engine_set_conv_grouped(h, b"backbone.body.layer1.0.conv2", 64, 8, wp, None, None) == -2
            msg = L.isegmi_last_error()
            assert word in msg and b"backbone.body.layer1.0.conv2" in msg, msg
        finally:
            L.isegmi_engine_destroy(h)
    h = engine(2)
    try:
        assert L.isegmi_engine_set_conv_grouped(h, b"x.conv2", 64, 16, wp, None, None) == -2      # 4 channels per group
        assert L.isegmi_engine_set_conv_grouped(h, b"x.conv2", 64, 1, wp, None, None) == -2       # groups 1 is set_conv's
        assert L.isegmi_engine_set_conv_grouped(h, b"x.conv2", 64, 8, wp, None, None) == 0
    finally:
        L.isegmi_engine_destroy(h)
