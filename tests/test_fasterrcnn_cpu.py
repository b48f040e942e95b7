"""Faster R-CNN (MODEL.MASK_ON False), class count and class-agnostic regression, host side: config mapping, seeded weights, importer
key sets, the box-only record block's layout, the category map, and the discrimination of the class-agnostic rule on the crafted input."""
import importlib.util
import os

import numpy as np
import pytest

import fasterrcnn_cases as fc
from conftest import ROOT
from oracle import ora


def _node(name, *opts):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", name))
    c.merge_from_list(list(opts))
    return c


@pytest.mark.parametrize("name,body,depth,pre,post,gn", [
    ("e2e_faster_rcnn_R_50_FPN_1x.yaml", "R-50-FPN", 50, 1000, 1000, False),
    ("e2e_faster_rcnn_R_101_FPN_1x.yaml", "R-101-FPN", 101, 1000, 1000, False),
    ("e2e_faster_rcnn_R_50_C4_1x.yaml", "R-50-C4", 50, 6000, 1000, False),
    ("e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml", "R-50-FPN", 50, 1000, 1000, True)])
def test_faster_rcnn_yamls_map_to_box_only_configs(name, body, depth, pre, post, gn):
    from isegmi.config import to_maskrcnn_config
    mc = to_maskrcnn_config(_node(name))
    assert mc.MASK_ON is False and mc.NUM_CLASSES == 81 and mc.CLS_AGNOSTIC_BBOX_REG is False
    assert mc.CONV_BODY == body and mc.depth == depth and mc.is_c4 == body.endswith("C4")
    assert (mc.RPN_PRE_NMS_TOP_N_TEST, mc.RPN_POST_NMS_TOP_N_TEST) == (pre, post)
    assert mc.USE_GN is gn and mc.BOX_HEAD == ("FPNXconv1fcFeatureExtractor" if gn else "FPN2MLPFeatureExtractor")
    assert mc.SIZE_DIVISIBILITY == (16 if mc.is_c4 else 32)


def test_the_three_head_keys_map_and_the_defaults_stay():
    from isegmi.config import cfg, to_maskrcnn_config
    from isegmi.maskrcnn import MaskRCNNConfig
    d = MaskRCNNConfig()
    assert d.MASK_ON is True and d.NUM_CLASSES == 81 and d.CLS_AGNOSTIC_BBOX_REG is False
    mc = to_maskrcnn_config(cfg.clone())                    # the project's default stays MASK_ON True (upstream's is False: DESIGN.md 13)
    assert mc.MASK_ON is True and mc.NUM_CLASSES == 81 and not mc.CLS_AGNOSTIC_BBOX_REG
    mc = to_maskrcnn_config(_node("e2e_mask_rcnn_R_50_FPN_1x.yaml"))
    assert mc.MASK_ON is True
    mc = to_maskrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9, "MODEL.CLS_AGNOSTIC_BBOX_REG", True))
    assert mc.NUM_CLASSES == 9 and mc.CLS_AGNOSTIC_BBOX_REG is True and mc.MASK_ON is False


@pytest.mark.parametrize("n", [1, 258])
def test_num_classes_outside_the_kernels_range_raises_naming_the_key(n):
    from isegmi.config import to_maskrcnn_config
    with pytest.raises(ValueError, match=r"MODEL\.ROI_BOX_HEAD\.NUM_CLASSES"):
        to_maskrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", n))
    for ok in (2, 257):
        assert to_maskrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", ok)).NUM_CLASSES == ok


def test_out_of_scope_keys_raise_by_name():
    from isegmi.config import to_maskrcnn_config
    for key in ("MODEL.RPN_ONLY", "MODEL.KEYPOINT_ON", "TEST.BBOX_AUG.ENABLED"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            to_maskrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_1x.yaml", key, True))
    with pytest.raises(ValueError, match="FPN2MLPFeatureExtractor"):   # GroupNorm with the 2-MLP head stays refused
        to_maskrcnn_config(_node("e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml", "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor"))


def test_gn_together_rule_leaves_the_mask_head_out_when_mask_is_off():
    """The GroupNorm faster_rcnn yaml never mentions ROI_MASK_HEAD.USE_GN (default False): accepted with MASK_ON False, and the very same node with
    MASK_ON True is refused for exactly that key."""
    from isegmi.config import to_maskrcnn_config
    c = _node("e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml")
    assert not c.MODEL.ROI_MASK_HEAD.USE_GN
    assert to_maskrcnn_config(c).USE_GN
    c.MODEL.ROI_MASK_HEAD.DILATION = 2          # not consulted either
    assert to_maskrcnn_config(c).USE_GN
    c.MODEL.ROI_MASK_HEAD.DILATION = 1
    c.MODEL.MASK_ON = True
    with pytest.raises(ValueError, match=r"MODEL\.ROI_MASK_HEAD\.USE_GN"):
        to_maskrcnn_config(c)
    c.MODEL.MASK_ON = False
    c.MODEL.FPN.USE_GN = False                  # the rule itself still holds over backbone + FPN + box head
    with pytest.raises(ValueError, match=r"MODEL\.FPN\.USE_GN"):
        to_maskrcnn_config(c)


# sha256 (fasterrcnn_cases.digest) of the three generators' output before they took mask / num_classes / cls_agnostic, recorded from that code
RECORDED = {
    (1234, "maskrcnn_state_dict"): "4e5f34f006f931c579d29461dfd932f3a00733d4e36377c27f5c5f8f2b384cf6",
    (1234, "maskrcnn_gn_state_dict"): "c7d37850cfebed14517d94c6b067b2df02d30fd10e4c8c98019b22896c02d154",
    (1234, "maskrcnn_c4_state_dict"): "ff76c372461971d5632ca17e213d7c15f3fb7603210e8113d91d875a6b4f5844",
    (77, "maskrcnn_state_dict"): "ef4b1d5af5949262996b35945785de566bb56b30b8df0b4e63128a953c27900c",
    (77, "maskrcnn_gn_state_dict"): "84eb1726dd0ee30e1d8b7daa5bc76de4f214925286cabc021b23db0e4a76d4b3",
    (77, "maskrcnn_c4_state_dict"): "8bc23a50f0b86a8f5e496f3649b8790d15384c02092c44db4388e720ab40ab5c",
}


@pytest.mark.parametrize("seed", [1234, 77])
@pytest.mark.parametrize("gen", ["maskrcnn_state_dict", "maskrcnn_gn_state_dict", "maskrcnn_c4_state_dict"])
def test_generator_defaults_are_byte_identical_and_mask_false_is_a_strict_subset(gen, seed):
    from isegmi import weights as W
    g = getattr(W, gen)
    full = g(seed)
    assert fc.digest(full) == RECORDED[(seed, gen)]
    assert fc.digest(g(seed, mask=True, num_classes=81, cls_agnostic=False)) == RECORDED[(seed, gen)]
    box = g(seed, mask=False)
    assert set(box) < set(full) and set(full) - set(box) == {k for k in full if k.startswith("roi_heads.mask.")}
    assert all(np.array_equal(box[k], full[k]) and box[k].dtype == full[k].dtype for k in box)
    assert "roi_heads.box.predictor.bbox_pred.weight" in box


def test_generators_size_the_predictors():
    from isegmi import weights as W
    cin = {"maskrcnn_state_dict": 1024, "maskrcnn_gn_state_dict": 1024, "maskrcnn_c4_state_dict": 2048}
    for gen, c in cin.items():
        sd = getattr(W, gen)(3, num_classes=9)
        assert sd["roi_heads.box.predictor.cls_score.weight"].shape == (9, c) and sd["roi_heads.box.predictor.bbox_pred.weight"].shape == (36, c)
        assert sd["roi_heads.mask.predictor.mask_fcn_logits.weight"].shape == (9, 256, 1, 1)
        sd = getattr(W, gen)(3, mask=False, num_classes=9, cls_agnostic=True)
        assert sd["roi_heads.box.predictor.bbox_pred.weight"].shape == (8, c) and sd["roi_heads.box.predictor.bbox_pred.bias"].shape == (8,)
        with pytest.raises(ValueError, match="NUM_CLASSES"):
            getattr(W, gen)(3, num_classes=258)


def test_random_weights_follow_the_config():
    import dataclasses
    from isegmi.maskrcnn import MaskRCNNConfig
    from isegmi.weights import maskrcnn_c4_state_dict, maskrcnn_state_dict, random_maskrcnn_state_dict
    a = random_maskrcnn_state_dict(dataclasses.replace(MaskRCNNConfig(), MASK_ON=False), 1234)
    assert fc.digest(a) == fc.digest(maskrcnn_state_dict(1234, mask=False))
    b = random_maskrcnn_state_dict(dataclasses.replace(MaskRCNNConfig.c4(), MASK_ON=False, NUM_CLASSES=5), 1234)
    assert fc.digest(b) == fc.digest(maskrcnn_c4_state_dict(1234, mask=False, num_classes=5))
    assert fc.digest(random_maskrcnn_state_dict(MaskRCNNConfig(), 1234)) == RECORDED[(1234, "maskrcnn_state_dict")]


def _importer():
    spec = importlib.util.spec_from_file_location("import_pth", os.path.join(ROOT, "tools", "import_pth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("family,mask_family", [("fasterrcnn_r50_fpn", "maskrcnn_r50_fpn"), ("fasterrcnn_r101_fpn", "maskrcnn_r101_fpn"),
                                                ("fasterrcnn_r50_c4", "maskrcnn_r50_c4"), ("fasterrcnn_r50_fpn_gn", "maskrcnn_r50_fpn_gn")])
def test_importer_families_have_no_mask_head(family, mask_family):
    mod = _importer()
    assert family in mod.FAMILIES
    box, full = mod.expected_keys(family), mod.expected_keys(mask_family)
    assert not [k for k in box if k.startswith("roi_heads.mask.")]
    assert {k: v for k, v in full.items() if not k.startswith("roi_heads.mask.")} == box
    assert box["roi_heads.box.predictor.cls_score.weight"][0] == 81 and box["roi_heads.box.predictor.bbox_pred.weight"][0] == 324
    sd = {k: np.zeros(s, np.float32) for k, s in box.items()}
    assert set(mod.convert(dict(sd), family)) == set(box)                       # a complete box-only checkpoint is accepted ...
    extra = dict(sd)
    extra["roi_heads.mask.predictor.mask_fcn_logits.bias"] = np.zeros(81, np.float32)
    with pytest.raises(KeyError, match="unused"):                                # ... a mask head in it is not part of the family
        mod.convert(extra, family)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [100, 128])
def test_box_only_block_layout(n, K):
    from isegmi.dist import coco_record_layout, unpack_coco_records
    secs, coff, total = coco_record_layout(n, K, 2, False, 0, box_only=True)
    assert list(secs) == ["status", "box", "count", "score", "label"]            # no str_off, no characters
    assert total == coff == fc.box_block_bytes(n, K)
    assert all(off % 8 == 0 for off, _, _, _ in secs.values()) and total % 8 == 0
    assert secs["status"][:2] == (0, 16) and secs["box"][0] == 16 and secs["box"][1] == n * K * 16
    assert secs["count"] == (16 + n * K * 16, n * 4, np.int32, (n,))
    ends = [off + nb for off, nb, _, _ in secs.values()]
    starts = [off for off, _, _, _ in secs.values()][1:] + [total]
    assert all(0 <= s - e < 8 for s, e in zip(starts, ends))                     # sections in order, less than 8 bytes of padding between them
    # a block written by hand comes back through unpack, and a zero block is an empty step
    rng = np.random.default_rng(n * 1000 + K)
    buf = np.zeros(total, np.uint8)
    vals = dict(box=rng.uniform(0, 500, (n, K, 4)).astype(np.float32), count=rng.integers(0, K + 1, n).astype(np.int32),
                score=rng.uniform(0, 1, (n, K)).astype(np.float32), label=rng.integers(1, 81, (n, K)).astype(np.int32))
    for k, v in vals.items():
        off, nb, dt, shp = secs[k]
        buf[off:off + nb] = v.view(np.uint8).ravel()
    rec = unpack_coco_records(buf, n, K, 2, box_only=True)
    assert rec["overflow"] is None and "str_off" not in rec and "chars" not in rec
    assert all(np.array_equal(rec[k], v) for k, v in vals.items())
    assert not unpack_coco_records(np.zeros(total, np.uint8), n, K, 2, box_only=True)["count"].any()
    # the mask block's layout is what it was
    msecs, mcoff, mtotal = coco_record_layout(n, K, 2, False, 64)
    assert "str_off" in msecs and mtotal == mcoff + 64


def test_category_map_and_bbox_only_results():
    from isegmi.coco import COCO_CATEGORY_IDS, label_categories, maskrcnn_results, results_from_records
    from isegmi.dist import coco_record_layout, unpack_coco_records
    c81 = label_categories(81)
    assert c81[1:] == list(COCO_CATEGORY_IDS) and c81[12] == 13 and c81[80] == 90 and c81[0] is None
    c9 = label_categories(9)
    assert c9[1:] == list(range(1, 9))                                           # any other count: the label is the category id
    own = label_categories(9, [11, 22, 33, 44, 55, 66, 77, 88])
    assert own[1] == 11 and own[8] == 88
    with pytest.raises(ValueError, match="category_ids"):
        label_categories(9, [1, 2, 3])
    assert label_categories(81, list(range(101, 181)))[80] == 180
    # host arrays -> results
    boxes = np.array([[10, 20, 49, 79], [1.5, 2.5, 3.5, 4.5]], np.float32)
    r = maskrcnn_results(7, boxes, [0.9, 0.4], [12, 1])
    assert [d["category_id"] for d in r] == [13, 1] and r[0]["bbox"] == [10.0, 20.0, 40.0, 60.0] and "segmentation" not in r[0]
    sc = np.array([0.9, 0.4], np.float32)
    r9 = maskrcnn_results(7, boxes, sc, [8, 3], categories=c9)
    assert [d["category_id"] for d in r9] == [8, 3]
    assert [d["category_id"] for d in maskrcnn_results(7, boxes, [0.9, 0.4], [8, 3], categories=own)] == [88, 33]
    # a box-only record block -> the same results, no `segmentation`
    n, K = 2, 100
    secs, _, total = coco_record_layout(n, K, 2, False, 0, box_only=True)
    buf = np.zeros(total, np.uint8)
    rec = unpack_coco_records(buf, n, K, 2, box_only=True)
    rec["box"][1, :2] = boxes; rec["count"][1] = 2; rec["score"][1, :2] = sc; rec["label"][1, :2] = [8, 3]
    res = results_from_records(rec, [5, 7], [(100, 100), (100, 100)], 2, K, categories=c9)
    assert res == r9 and all("segmentation" not in d for d in res)
    assert results_from_records(rec, [5, None], [(100, 100), (1, 1)], 2, K, categories=c9) == []


def test_class_agnostic_rule_discriminates_on_the_crafted_input():
    """ora.box_postprocess on regr = tile(reg[:, 4:8], ncls) -- the class-agnostic rule -- against the per-class reading of the same eight-wide rows:
    the answers differ, so the GPU comparison against the tiled oracle (tests/test_fasterrcnn_ops_gpu.py) can fail."""
    c = fc.crafted()
    ncls, (h, w) = c["ncls"], c["hw"]
    tiled = fc.agnostic_regr(c["reg8"], ncls)
    assert tiled.shape == (3, 4 * ncls) and np.array_equal(tiled[:, 8:12], c["reg8"][:, 4:8]) and np.array_equal(tiled[:, 0:4], c["reg8"][:, 4:8])
    ab, as_, al = ora.box_postprocess(c["logits"], tiled, c["props"], float(w), float(h))
    pc = fc.per_class_reading(c["reg8"], ncls)
    assert np.array_equal(pc[:, :8], c["reg8"]) and np.array_equal(pc[0, 8:], c["reg8"][1, :4])
    pb, ps, pl = ora.box_postprocess(c["logits"], pc, c["props"], float(w), float(h))
    assert len(as_) >= 2 and set(al.tolist()) == {1, 2}
    assert (len(as_), len(ps)) == (2, 3)          # agnostic: proposals 0 and 1 stay on top of each other, one is suppressed; per-class: pushed apart, both kept
    assert not np.array_equal(ab[: len(pb)], pb[: len(ab)])
    # class 1 reads 4..7 under both rules: its box is the same -- the difference is class 2's alone
    assert np.array_equal(ab[al == 1], pb[pl == 1])


def _dry_load(sd, cfg):
    """MaskRCNN's loaders with the device calls recorded instead of executed; the state dict records which keys were read."""
    from isegmi.maskrcnn import MaskRCNN

    class Tracking(dict):
        def __init__(self, *a):
            super().__init__(*a)
            self.read = set()

        def __getitem__(self, k):
            self.read.add(k)
            return super().__getitem__(k)

    m = object.__new__(MaskRCNN)
    m.cfg, m.H, m.W, m._h = cfg, 64, 96, None
    m.convs, m.tensors, m.params = {}, {}, {}
    m._set_conv_krsc = lambda name, w, scale=None, shift=None: m.convs.__setitem__(name, np.asarray(w).shape)
    m._set_tensor = lambda name, a: m.tensors.__setitem__(name, np.asarray(a).shape)
    m.set_param = lambda name, value: m.params.__setitem__(name, value)
    t = Tracking(sd)
    (m._load_c4 if cfg.is_c4 else m._load_gn if cfg.USE_GN else m._load)(t)
    return m, t


@pytest.mark.parametrize("kind", ["fpn", "gn", "c4"])
def test_loaders_take_mask_less_dicts_and_size_the_predictor(kind):
    import dataclasses
    from isegmi import weights as W
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    base = {"fpn": MaskRCNNConfig(), "c4": MaskRCNNConfig.c4(),
            "gn": dataclasses.replace(MaskRCNNConfig(), USE_GN=True, STRIDE_IN_1X1=False, BOX_HEAD="FPNXconv1fcFeatureExtractor")}[kind]
    gen = {"fpn": W.maskrcnn_state_dict, "gn": W.maskrcnn_gn_state_dict, "c4": W.maskrcnn_c4_state_dict}[kind]
    cin = 2048 if kind == "c4" else 1024
    box_cfg = dataclasses.replace(base, MASK_ON=False)
    m, t = _dry_load(gen(3, mask=False), box_cfg)
    assert t.read == set(t) and m.convs["roi_heads.box.predictor.cls_bbox"] == (405, 1, 1, cin)          # every tensor of the box-only dict is consumed
    assert not [k for k in list(m.convs) + list(m.tensors) if "mask" in k] and m.has_mask_head is False
    full = gen(3)
    m, t = _dry_load(full, box_cfg)                                                                      # present mask keys are ignored
    assert not [k for k in t.read if k.startswith("roi_heads.mask.")] and not [k for k in list(m.convs) + list(m.tensors) if "mask" in k]
    m, t = _dry_load(full, base)                                                                         # and the mask model loads what it loaded
    assert m.has_mask_head and m.tensors["mask_logits.w"] == (81, 256) and "roi_heads.mask.predictor.conv5_mask.3" in m.convs
    with pytest.raises(ValueError, match=r"MODEL\.MASK_ON"):
        _dry_load(gen(3, mask=False), base)
    with pytest.raises(ValueError, match=r"MODEL\.MASK_ON"):                                             # the constructor refuses before any device call
        MaskRCNN(gen(3, mask=False), 64, 96, cfg=base, max_batch=1)
    # class count and the class-agnostic form
    m, _ = _dry_load(gen(3, num_classes=9), dataclasses.replace(base, NUM_CLASSES=9))
    assert m.convs["roi_heads.box.predictor.cls_bbox"] == (45, 1, 1, cin) and m.tensors["mask_logits.w"] == (9, 256) and m.tensors["mask_logits.b"] == (9,)
    m, _ = _dry_load(gen(3, mask=False, num_classes=9, cls_agnostic=True), dataclasses.replace(box_cfg, NUM_CLASSES=9, CLS_AGNOSTIC_BBOX_REG=True))
    assert m.convs["roi_heads.box.predictor.cls_bbox"] == (17, 1, 1, cin)
    with pytest.raises(ValueError, match=r"bbox_pred has 8 outputs: 9 classes need 36 = 4 \* NUM_CLASSES"):
        _dry_load(gen(3, mask=False, num_classes=9, cls_agnostic=True), dataclasses.replace(box_cfg, NUM_CLASSES=9))
    with pytest.raises(ValueError, match=r"cls_score has 81 outputs, MODEL\.ROI_BOX_HEAD\.NUM_CLASSES is 9"):
        _dry_load(gen(3, mask=False), dataclasses.replace(box_cfg, NUM_CLASSES=9))
    with pytest.raises(ValueError, match=r"MODEL\.ROI_BOX_HEAD\.NUM_CLASSES"):
        MaskRCNN(gen(3, mask=False), 64, 96, cfg=dataclasses.replace(box_cfg, NUM_CLASSES=258), max_batch=1)
