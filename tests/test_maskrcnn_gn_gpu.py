"""The GroupNorm Mask R-CNN (gn_baselines: GN backbone, FPN, Xconv1fc box head, GN mask head) end to end: the HIP engine against
tests/maskrcnn_gn_ref.py -- the oracle's ops plus the GroupNorm restatement in the kernel's summation order -- bit for bit."""
import numpy as np
import pytest

import groupnorm_ref as G
from maskrcnn_gn_common import MaskRCNNGNRef, gn_cfg as _cfg, sd, small  # noqa: F401  (sd, small: fixtures, shared with test_maskrcnn_gn_forms_gpu.py)

pytestmark = pytest.mark.gpu


def _same_detections(out, rd):
    for bl, r in zip(out, rd):
        assert len(bl) == len(r["score"])
        assert np.array_equal(bl.get_field("labels"), r["label"].astype(np.int64))
        assert np.array_equal(bl.get_field("scores"), r["score"]) and np.array_equal(bl.bbox, r["box"])
        assert np.array_equal(bl.get_field("mask")[:, 0], r["mask28"])


def test_gn_small_batch2_bit_exact(ffi, sd, small):
    from isegmi.maskrcnn import MaskRCNN
    x, hw, ref, rd = small
    assert x.shape == (2, 256, 352, 3)
    assert max(len(r["score"]) for r in rd) >= 8, "the seeded weights must exercise the mask head"
    model = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=_cfg(), max_batch=2)
    out = model(x, hw)
    assert np.array_equal(model.fetch("res2.C", 2), ref.feats["C2"])
    for name in ("P2", "P3", "P4", "P5", "P6"):
        assert np.array_equal(model.fetch(name, 2), ref.feats[name]), name
    pc = model.fetch("proposal_count", 2); pr = model.fetch("proposals", 2); ps = model.fetch("proposal_scores", 2)
    xf = model.fetch("box.xconv3", 2 * 1000).reshape(2, 1000, 7, 7, 256)
    for n in range(2):
        r = rd[n]
        assert pc[n] == len(r["proposals"])
        assert np.array_equal(ps[n, : pc[n]], r["proposal_scores"]) and np.array_equal(pr[n, : pc[n]], r["proposals"])
        assert np.array_equal(xf[n, : pc[n]], r["xconv"])
    _same_detections(out, rd)
    model.paste_device(256, 352); model.sync()
    masks = model.fetch("det.masks", 2)
    for n in range(2):
        rm, _ = MaskRCNNGNRef.paste(rd[n], 256, 352)
        assert rm.any() and np.array_equal(masks[n, : len(rm)], rm)
    model.close()


def test_gn_hipgraph_replay_equals_eager(ffi, sd, small):
    from isegmi.maskrcnn import MaskRCNN
    x, hw, _, rd = small
    model = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=_cfg(), max_batch=2)
    _same_detections(model(x, hw), rd)
    model.set_param("graph", 1.0)
    for _ in range(4):   # warm-up, capture, replays
        out = model(x, hw)
        _same_detections(out, rd)
    cap, rep, fail = (ffi.C.c_int64() for _ in range(3))
    ffi.check(ffi.lib().isegmi_engine_graph_stats(model._h, ffi.C.byref(cap), ffi.C.byref(rep), ffi.C.byref(fail)))
    assert cap.value >= 1 and rep.value >= 1 and fail.value == 0, (cap.value, rep.value, fail.value)
    model.close()


def test_gn_no_detections(ffi, sd):
    """Nothing passes SCORE_THRESH: both heads run over zero detections, empty BoxList, paste writes nothing."""
    from isegmi.maskrcnn import MaskRCNN, prepare_images
    sd2 = dict(sd)
    b = sd["roi_heads.box.predictor.cls_score.bias"].copy(); b[0] += 50.0
    sd2["roi_heads.box.predictor.cls_score.bias"] = b
    rng = np.random.default_rng(9)
    x, hw = prepare_images([rng.uniform(0, 255, (200, 230, 3)).astype(np.float32)])
    model = MaskRCNN(sd2, x.shape[1], x.shape[2], cfg=_cfg(), max_batch=1)
    out = model(x, hw)
    assert len(out[0]) == 0
    model.paste_device(x.shape[1], x.shape[2]); model.sync()
    assert not model.fetch("det.masks", 1).any()
    model.close()


def test_gn_and_frozenbn_models_side_by_side(ffi, sd, small):
    """A FrozenBN model and a GroupNorm model in one process, run alternately: neither disturbs the other."""
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.weights import maskrcnn_state_dict
    x, hw, _, rd = small
    bn = MaskRCNN(maskrcnn_state_dict(1234), x.shape[1], x.shape[2], max_batch=2)
    first = bn(x, hw)
    gn = MaskRCNN(sd, x.shape[1], x.shape[2], cfg=_cfg(), max_batch=2)
    _same_detections(gn(x, hw), rd)
    again = bn(x, hw)
    _same_detections(gn(x, hw), rd)
    assert sum(len(b) for b in first) > 0
    for a, b in zip(first, again):
        assert np.array_equal(a.bbox, b.bbox) and np.array_equal(a.get_field("scores"), b.get_field("scores"))
        assert np.array_equal(a.get_field("mask"), b.get_field("mask"))
    bn.close(); gn.close()


def test_gn_fp16_is_refused(ffi, sd):
    from isegmi.maskrcnn import MaskRCNN
    with pytest.raises(ValueError, match="fp16"):
        MaskRCNN(sd, 256, 352, cfg=_cfg(), max_batch=1, fp16=True)


def test_gn_launches_at_full_size_shapes(ffi):
    """The CPU reference of a whole 800x1344 bs = 2 forward takes minutes, so the full-size check is op by op: every distinct GroupNorm launch shape of
    that forward (stem, one layer of res2..res5, P2, the box head at 1000 RoIs per image, the mask head at 100), bit-exact against the restatement."""
    rng = np.random.default_rng(11)
    for N, H, W, C in ((2, 400, 672, 64), (2, 200, 336, 64), (2, 200, 336, 256), (2, 100, 168, 512), (2, 50, 84, 1024), (2, 25, 42, 2048),
                       (2000, 7, 7, 256), (200, 14, 14, 256)):
        x = rng.standard_normal((N, H, W, C), np.float32)
        ga = rng.uniform(0.5, 1.5, C).astype(np.float32); be = (rng.standard_normal(C) * 0.1).astype(np.float32)
        assert np.array_equal(ffi.group_norm(x, 32, ga, be, relu=True), G.gn_kernel_order(x, 32, ga, be, relu=True)), (N, H, W, C)


def test_cli_test_net_runs_the_gn_yaml(ffi, tmp_path):
    """`python -m isegmi.cli test_net --config-file configs/e2e_mask_rcnn_R_50_FPN_1x_gn.yaml MODEL.WEIGHT random` end to end (at a small test size)."""
    import json
    import os
    from PIL import Image
    from isegmi import cli
    rng = np.random.default_rng(3)
    src = tmp_path / "in"; src.mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (90 + 10 * i, 120, 3)).astype(np.uint8)).save(src / ("im%d.png" % i))
    yaml = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "e2e_mask_rcnn_R_50_FPN_1x_gn.yaml")
    out = cli.main(["test_net", "--config-file", yaml, "--images", str(src), "--output", str(tmp_path / "m.json"),
                    "MODEL.WEIGHT", "random", "INPUT.MIN_SIZE_TEST", "160", "INPUT.MAX_SIZE_TEST", "256"])
    back = json.load(open(tmp_path / "m.json"))
    assert len(back) == len(out) > 0 and {r["image_id"] for r in back} <= {0, 1}
    assert all(set(r) >= {"image_id", "category_id", "bbox", "score", "segmentation"} for r in back)
