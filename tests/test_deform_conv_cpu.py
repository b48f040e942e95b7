"""The deformable-convolution feature without a GPU: the operator reference and its crafted cases (each case reaches the limit it is named
after, and each WRONG sampling rule gives different bits on it), the K order the fused kernel must walk, the config mapping with every refusal, the seeded
state dicts, the importer families and the loader's shape refusals."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import deform_conv_cases as dc
from oracle import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAMLS = {"e2e_mask_rcnn_dconv_R_50_FPN_1x.yaml": (True, False), "e2e_mask_rcnn_mdconv_R_50_FPN_1x.yaml": (True, True),
         "e2e_faster_rcnn_dconv_R_50_FPN_1x.yaml": (False, False), "e2e_faster_rcnn_mdconv_R_50_FPN_1x.yaml": (False, True)}
# sha256 over (name, dtype, shape, bytes) of maskrcnn_state_dict(1234, 50), names sorted, computed on the commit BEFORE the deformable layers were added
PARENT_R50_DIGEST = "4e5f34f006f931c579d29461dfd932f3a00733d4e36377c27f5c5f8f2b384cf6"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- the sampling rule ----------------------------------------------------------------------------------------------------------------------------------
def _rule_case(seed=5, H=6, W=8, C=8, stride=1):
    rng = np.random.default_rng(seed)
    Ho, Wo = dc.out_hw(H, W, stride)
    x = rng.uniform(0.5, 1.5, (2, H, W, C)).astype(np.float32)
    om = rng.normal(0, 1.5, (2, Ho, Wo, 27)).astype(np.float32)
    return x, om


@pytest.mark.parametrize("stride", [1, 2])
def test_numpy_restatement_equals_the_oracle(stride):
    x, om = _rule_case(stride=stride)
    assert _same(dc.sample_np(x, om, stride), ora.deform_im2col(x, om, 3, 3, stride, 1, 1))
    for kind in dc.CRAFTED:
        c, ref, col, want = dc.crafted(kind, True)
        assert _same(dc.sample_np(c["x"], c["om"], 1), col), kind


@pytest.mark.parametrize("rule", ["swap_yx", "ignore_mask", "mask_at_2k"])
def test_wrong_rule_gives_different_bits(rule):
    """Swapped dy / dx, the mask ignored, the mask logit read at channel 2k instead of 18 + k: each changes the columns of a random case."""
    x, om = _rule_case()
    right = ora.deform_im2col(x, om, 3, 3, 1, 1, 1)
    wrong = dc.sample_np(x, om, 1, **{rule: True})
    assert wrong.shape == right.shape and not np.array_equal(_bits(wrong), _bits(right))
    assert float(np.abs(wrong - right).max()) > 1e-2   # not a rounding difference


def test_border_at_minus_one_is_strict():
    """A position exactly on h = -1 is excluded.  With `>=` it would be sampled with hl = -1, lh = 0: finite features still give 0 (weights 0 on the live
    corners), so the case that tells the rules apart has a non-finite feature in row 0 -- `>` gives +0, `>=` gives 0 * inf = NaN."""
    c, ref, col, want = dc.crafted("on_minus1_and_H", True)
    assert want == dc.CH * dc.CW * 9 == dc.zero_rows(col, dc.CC)
    x = np.array(c["x"]); x[0, 0, 2, :] = np.inf
    right = ora.deform_im2col(x, c["om"], 3, 3, 1, 1, 1)
    assert not right.any() and _same(right, dc.sample_np(x, c["om"], 1))
    assert np.isnan(dc.sample_np(x, c["om"], 1, ge_border=True)).any()


@pytest.mark.parametrize("modulated", [True, False])
@pytest.mark.parametrize("kind", dc.CRAFTED)
def test_crafted_cases_reach_their_limit(kind, modulated):
    c, ref, col, want = dc.crafted(kind, modulated)
    rows = dc.CH * dc.CW * 9
    assert dc.zero_rows(col, dc.CC) == want == dc.dead_rows(c["om"], dc.CH, dc.CW, 1)
    h, w = dc.positions(c["om"], dc.CH, dc.CW, 1)
    if kind == "integer":
        assert np.array_equal(h, np.floor(h)) and np.array_equal(w, np.floor(w)) and 0 < want < rows
    elif kind == "on_minus1_and_H":
        assert set(np.unique(h)) == {-1.0, float(dc.CH)} and want == rows and not col.any()
    elif kind == "last_row_col":
        assert (h == dc.CH - 1).all() and (w == dc.CW - 1).all() and want == 0
        m = ora.map_f32(np.ascontiguousarray(dc.as27(c["om"])[..., 18:]), 1)
        corner = c["x"][0, dc.CH - 1, dc.CW - 1]
        assert _same(col.reshape(1, dc.CH, dc.CW, 9, dc.CC), np.broadcast_to(corner, (1, dc.CH, dc.CW, 9, dc.CC)) * m[..., None])
    elif kind == "between_minus1_and_0":
        assert ((h > -1) & (h < 0)).all() and want == 0
        m = ora.map_f32(np.ascontiguousarray(dc.as27(c["om"])[..., 18:]), 1)
        lower = (np.float32(0.5) * np.float32(0.75)) * c["x"][0, 0, 2] + (np.float32(0.5) * np.float32(0.25)) * c["x"][0, 0, 3]   # the two upper corners are outside
        assert _same(col.reshape(1, dc.CH, dc.CW, 9, dc.CC), np.broadcast_to(lower, (1, dc.CH, dc.CW, 9, dc.CC)) * m[..., None])
    elif kind == "huge":
        assert (np.abs(h) > 9e5).all() and want == rows and not col.any()
    elif kind == "nonfinite":
        assert np.isnan(h).any() and np.isposinf(h).any() and np.isneginf(h).any() and np.isnan(w).any() and np.isinf(w).any()
        assert want == 239 and not np.isnan(col).any()
    else:
        assert not col.reshape(dc.CH, dc.CW, 9 * dc.CC)[2, 3].any()
        y = ref[0, 2, 3]
        assert _same(y, np.maximum(c["shift"], np.float32(0)))   # every tap of the pixel outside: fmaf(+0, scale, shift) -> ReLU
        assert (ref[0, 2, 4] != np.maximum(c["shift"], np.float32(0))).any()


def test_saturated_logit_reproduces_the_unmodulated_columns():
    """dm_sigmoid(+100) is exactly 1.0 and v * 1.0 is exact: the 27-channel oracle fed +100 logits IS the DCNv1 reference."""
    assert ora.map_f32(np.asarray([dc.SAT], np.float32), 1)[0] == np.float32(1.0)
    x, om = _rule_case()
    off = np.ascontiguousarray(om[..., :18])
    assert _same(dc.columns(x, off, 1), dc.sample_np(x, off, 1, ignore_mask=True))
    assert not _same(dc.columns(x, off, 1), dc.columns(x, om, 1))


def test_k_order_of_the_columns_is_not_the_plain_3x3_walk():
    """C = 256: a plain 3x3 walks 128-channel K groups outermost (conv_korder.h), a 1x1 over the columns walks (tap, channel).  On zero offsets with a
    saturated mask the columns ARE the plain im2col, so the two convolutions sum the same products in different orders -- and differ in some output."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1, 6, 6, 256)).astype(np.float32)
    w = (rng.standard_normal((32, 3, 3, 256)) / 48.0).astype(np.float32)
    om = np.zeros((1, 6, 6, 27), np.float32); om[..., 18:] = dc.SAT
    col = ora.deform_im2col(x, om, 3, 3, 1, 1, 1)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    plain_cols = np.concatenate([xp[:, i:i + 6, j:j + 6] for i in range(3) for j in range(3)], -1)
    assert _same(col, plain_cols)
    as_1x1 = ora.conv2d(col, w.reshape(32, 1, 1, 9 * 256), 1, 0)
    as_3x3 = ora.conv2d(x, w, 1, 1)
    assert as_1x1.shape == as_3x3.shape
    assert not np.array_equal(_bits(as_1x1), _bits(as_3x3)), "the two K orders must differ in at least one output"
    assert np.allclose(as_1x1, as_3x3, rtol=0, atol=1e-4)
    # at C = 64 (one K group) the two orders coincide: the difference above is the order, nothing else
    assert _same(ora.conv2d(np.ascontiguousarray(plain_cols.reshape(1, 6, 6, 9, 256)[..., :64]).reshape(1, 6, 6, 576), np.ascontiguousarray(w[..., :64]).reshape(32, 1, 1, 576), 1, 0),
                 ora.conv2d(np.ascontiguousarray(x[..., :64]), np.ascontiguousarray(w[..., :64]), 1, 1))


def test_random_references_cover_the_listed_shapes():
    shapes = dc.RANDOM_SHAPES
    assert {s[:3] for s in shapes} >= {(1, 1, 1), (1, 5, 7), (2, 9, 13), (1, 1, dc.TILE - 1), (1, 1, dc.TILE), (1, 1, dc.TILE + 1)}
    assert {s[3] for s in shapes} == {32, 64, 160, 256} and {s[4] for s in shapes} == {4, 32, 96, 260, 516}
    assert {s[5] for s in shapes} == {1, 2} and {s[6] for s in shapes} == {0, 1} and {s[7] for s in shapes} == {0, 1}
    c, ref, col = dc.random_reference(4)   # (1, 5, 7) stride 1: some taps leave the image, most do not
    z = dc.zero_rows(col, 32)
    assert 0 < z < 5 * 7 * 9 and z == dc.dead_rows(c["om"], 5, 7, 1)


# ---- configuration --------------------------------------------------------------------------------------------------------------------------------------
def _cfg(**keys):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_list([v for kv in keys.items() for v in kv])
    return c


def test_defaults_and_mapping():
    from isegmi.config import cfg, to_maskrcnn_config
    rn = cfg.MODEL.RESNETS
    assert tuple(rn.STAGE_WITH_DCN) == (False,) * 4 and rn.WITH_MODULATED_DCN is False and rn.DEFORMABLE_GROUPS == 1
    mc = to_maskrcnn_config(cfg.clone())
    assert mc.STAGE_WITH_DCN == (False,) * 4 and not mc.WITH_MODULATED_DCN
    for body, depth in (("R-50-FPN", 50), ("R-101-FPN", 101)):
        for stages in ((False, True, True, True), (True, False, False, False), (False, False, False, True), (True, True, True, True)):
            for mod in (False, True):
                for mask in (False, True):
                    mc = to_maskrcnn_config(_cfg(**{"MODEL.BACKBONE.CONV_BODY": body, "MODEL.RESNETS.STAGE_WITH_DCN": str(stages),
                                                    "MODEL.RESNETS.WITH_MODULATED_DCN": str(mod), "MODEL.MASK_ON": str(mask)}))
                    assert (mc.STAGE_WITH_DCN, mc.WITH_MODULATED_DCN, mc.MASK_ON, mc.depth) == (stages, mod, mask, depth)
    # WITH_MODULATED_DCN without a deformable stage builds the plain model, as upstream
    assert to_maskrcnn_config(_cfg(**{"MODEL.RESNETS.WITH_MODULATED_DCN": "True"})) == to_maskrcnn_config(cfg.clone())


@pytest.mark.parametrize("name", sorted(YAMLS))
def test_shipped_yamls_map(name):
    from isegmi.config import cfg, to_maskrcnn_config
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", name))
    mc = to_maskrcnn_config(c)
    mask, mod = YAMLS[name]
    assert mc.STAGE_WITH_DCN == (False, True, True, True) and mc.WITH_MODULATED_DCN is mod and mc.MASK_ON is mask
    assert mc.depth == 50 and mc.CONV_BODY == "R-50-FPN" and not mc.USE_GN and mc.NUM_GROUPS == 1
    assert "MASK_ON: %s" % mask in open(os.path.join(ROOT, "configs", name)).read()


DCN = {"MODEL.RESNETS.STAGE_WITH_DCN": "(False, True, True, True)"}
GN = {"MODEL.RESNETS.TRANS_FUNC": "BottleneckWithGN", "MODEL.RESNETS.STEM_FUNC": "StemWithGN", "MODEL.FPN.USE_GN": "True", "MODEL.ROI_BOX_HEAD.USE_GN": "True",
      "MODEL.ROI_MASK_HEAD.USE_GN": "True", "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR": "FPNXconv1fcFeatureExtractor", "MODEL.RESNETS.STRIDE_IN_1X1": "False"}


@pytest.mark.parametrize("keys, word", [
    ({"MODEL.RESNETS.DEFORMABLE_GROUPS": "2"}, "DEFORMABLE_GROUPS"),
    (dict(DCN, **{"MODEL.RESNETS.DEFORMABLE_GROUPS": "4"}), "DEFORMABLE_GROUPS"),
    (dict(DCN, **GN), "STAGE_WITH_DCN.*GroupNorm"),
    (dict(DCN, **{"MODEL.RESNETS.NUM_GROUPS": "32", "MODEL.RESNETS.WIDTH_PER_GROUP": "8", "MODEL.RESNETS.STRIDE_IN_1X1": "False", "MODEL.BACKBONE.CONV_BODY": "R-101-FPN"}),
     "STAGE_WITH_DCN.*NUM_GROUPS"),
    (dict(DCN, **{"MODEL.BACKBONE.CONV_BODY": "R-50-C4"}), "STAGE_WITH_DCN.*R-50-C4"),
    ({"MODEL.RESNETS.STAGE_WITH_DCN": "(True, True)"}, "STAGE_WITH_DCN.*four"),
])
def test_two_stage_refusals_name_the_key(keys, word):
    from isegmi.config import to_maskrcnn_config
    with pytest.raises(ValueError, match=word):
        to_maskrcnn_config(_cfg(**keys))


def test_keypoint_and_retinanet_refuse_dcn():
    from isegmi.config import to_keypointrcnn_config, to_retinanet_config
    with pytest.raises(ValueError, match="STAGE_WITH_DCN.*KEYPOINT_ON"):
        to_keypointrcnn_config(_cfg(**dict(DCN, **{"MODEL.KEYPOINT_ON": "True", "MODEL.MASK_ON": "False", "MODEL.ROI_BOX_HEAD.NUM_CLASSES": "2"})))
    retina = {"MODEL.RETINANET_ON": "True", "MODEL.MASK_ON": "False", "MODEL.BACKBONE.CONV_BODY": "R-50-FPN-RETINANET"}
    with pytest.raises(ValueError, match="STAGE_WITH_DCN.*RETINANET_ON"):
        to_retinanet_config(_cfg(**dict(DCN, **retina)))
    with pytest.raises(ValueError, match="DEFORMABLE_GROUPS"):
        to_retinanet_config(_cfg(**dict(retina, **{"MODEL.RESNETS.DEFORMABLE_GROUPS": "2"})))
    to_retinanet_config(_cfg(**retina))   # and the plain model still maps


def test_model_class_refusals_before_any_device_call():
    """MaskRCNN(...) refuses fp16, the C4 body, GroupNorm, ResNeXt and the keypoint head next to deformable stages before an engine exists."""
    import dataclasses
    import maskrcnn_dcn_ref as mr
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    sd = {}   # never read: the refusals come first
    with pytest.raises(ValueError, match="STAGE_WITH_DCN.*fp16"):
        MaskRCNN(sd, 64, 96, cfg=mr.config(), fp16=True)
    for kw, word in ((dict(USE_GN=True, BOX_HEAD="FPNXconv1fcFeatureExtractor"), "GroupNorm"), (dict(NUM_GROUPS=32, WIDTH_PER_GROUP=8), "NUM_GROUPS"),
                     (dict(KEYPOINT_ON=True, MASK_ON=False, NUM_CLASSES=2), "KEYPOINT_ON")):
        with pytest.raises(ValueError, match="STAGE_WITH_DCN.*" + word):
            MaskRCNN(sd, 64, 96, cfg=mr.config(**kw))
    c4 = dataclasses.replace(MaskRCNNConfig.c4(), STAGE_WITH_DCN=(False, True, True, False))
    with pytest.raises(ValueError, match="STAGE_WITH_DCN.*C4"):
        MaskRCNN(sd, 64, 96, cfg=c4)


# ---- state dicts, importer, loader ----------------------------------------------------------------------------------------------------------------------
def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode()); h.update(str(sd[k].dtype).encode()); h.update(str(sd[k].shape).encode()); h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def test_state_dict_generator_keeps_the_plain_dict_and_adds_the_deformable_layers():
    from isegmi.weights import YOLACT_DCN_OFFSET_STD, maskrcnn_state_dict, random_maskrcnn_state_dict
    import maskrcnn_dcn_ref as mr
    plain = maskrcnn_state_dict(1234, 50)
    assert _digest(plain) == PARENT_R50_DIGEST
    for mod in (False, True):
        sd = maskrcnn_state_dict(1234, 50, stage_with_dcn=(0, 1, 1, 1), modulated=mod)
        oc = 27 if mod else 18
        moved = {k for k in plain if ".conv2.weight" in k and not k.startswith("backbone.body.layer1.")}
        assert len(moved) == 4 + 6 + 3
        for k in plain:
            k2 = k.replace(".conv2.weight", ".conv2.conv.weight") if k in moved else k
            assert np.array_equal(sd[k2], plain[k]), k
        extra = set(sd) - {k.replace(".conv2.weight", ".conv2.conv.weight") if k in moved else k for k in plain}
        assert extra == {k[:-len("weight")] + "offset." + s for k in moved for s in ("weight", "bias")}
        for li, planes in ((2, 128), (3, 256), (4, 512)):
            w = sd["backbone.body.layer%d.0.conv2.offset.weight" % li]
            assert w.shape == (oc, planes, 3, 3) and sd["backbone.body.layer%d.0.conv2.offset.bias" % li].shape == (oc,)
            assert float(w.std() * np.sqrt(9.0 * planes)) == pytest.approx(YOLACT_DCN_OFFSET_STD, rel=0.05)
        assert "backbone.body.layer1.0.conv2.weight" in sd and "backbone.body.layer2.0.conv2.weight" not in sd
        rnd = random_maskrcnn_state_dict(mr.config(modulated=mod), 1234)
        assert _digest(rnd) == _digest(sd)
    one = maskrcnn_state_dict(1234, 50, mask=False, stage_with_dcn=(1, 0, 0, 0))
    assert "backbone.body.layer1.2.conv2.offset.weight" in one and "backbone.body.layer2.0.conv2.weight" in one and not any(k.startswith("roi_heads.mask") for k in one)
    with pytest.raises(ValueError, match="stage_with_dcn"):
        maskrcnn_state_dict(1234, 50, stage_with_dcn=(1, 1))
    with pytest.raises(ValueError, match="deformable"):
        maskrcnn_state_dict(1234, 50, gn=True, stage_with_dcn=(0, 1, 1, 1))


def _importer():
    spec = importlib.util.spec_from_file_location("import_pth", os.path.join(ROOT, "tools", "import_pth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Tracking(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


def _dry_load(sd, cfg):
    """MaskRCNN._load with the device calls recorded instead of executed."""
    from isegmi.maskrcnn import MaskRCNN
    m = object.__new__(MaskRCNN)
    m.cfg, m.H, m.W, m._h = cfg, 64, 96, None
    m.convs, m.tensors, m.params = {}, {}, {}
    m._set_conv_krsc = lambda name, w, scale=None, shift=None: m.convs.__setitem__(name, (np.asarray(w).shape, None if shift is None else np.asarray(shift).shape))
    m._set_tensor = lambda name, a: m.tensors.__setitem__(name, np.asarray(a).shape)
    m.set_param = lambda name, value: m.params.__setitem__(name, value)
    t = _Tracking(sd)
    m._load(t)
    return m, t


FAMILIES = {"maskrcnn_dconv_r50_fpn": (True, False), "maskrcnn_mdconv_r50_fpn": (True, True), "fasterrcnn_dconv_r50_fpn": (False, False),
            "fasterrcnn_mdconv_r50_fpn": (False, True)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_importer_round_trip(family):
    import maskrcnn_dcn_ref as mr
    from isegmi.weights import maskrcnn_state_dict
    mod = _importer()
    assert family in mod.FAMILIES
    mask, modulated = FAMILIES[family]
    sd = maskrcnn_state_dict(7, 50, mask=mask, stage_with_dcn=(0, 1, 1, 1), modulated=modulated)
    ck = {"model": {"module." + k: v for k, v in sd.items()}, "iteration": 90000}
    out = mod.convert(ck, family)
    assert set(out) == set(sd) and all(np.array_equal(out[k], sd[k]) for k in sd)
    m, t = _dry_load(out, mr.config(modulated=modulated, MASK_ON=mask))
    assert t.read == set(out), sorted(set(out) - t.read)[:5]
    oc = 27 if modulated else 18
    assert m.convs["backbone.body.layer3.5.conv2.conv_offset_mask"] == ((oc, 3, 3, 256), (oc,))
    assert m.convs["backbone.body.layer3.5.conv2"] == ((256, 1, 1, 9 * 256), (256,))
    assert m.convs["backbone.body.layer1.0.conv2"][0] == (64, 3, 3, 64) and "backbone.body.layer1.0.conv2.conv_offset_mask" not in m.convs
    # the wrong family raises: the other DCN version (shape), the other head (keys), the plain model (keys)
    other = family.replace("_mdconv_", "_X_").replace("_dconv_", "_mdconv_").replace("_X_", "_dconv_")
    with pytest.raises(ValueError, match="shape mismatch"):
        mod.convert(ck, other)
    with pytest.raises(KeyError):
        mod.convert(ck, "maskrcnn_r50_fpn" if mask else "fasterrcnn_r50_fpn")
    with pytest.raises(KeyError):
        mod.convert(ck, family.replace("maskrcnn", "X").replace("fasterrcnn", "maskrcnn").replace("X", "fasterrcnn"))


def test_loader_shape_refusals_name_the_key():
    import maskrcnn_dcn_ref as mr
    from isegmi.maskrcnn import MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    md = maskrcnn_state_dict(7, 50, stage_with_dcn=(0, 1, 1, 1), modulated=True)
    d1 = maskrcnn_state_dict(7, 50, stage_with_dcn=(0, 1, 1, 1), modulated=False)
    plain = maskrcnn_state_dict(7, 50)
    with pytest.raises(ValueError, match=r"layer2\.0\.conv2\.offset\.weight.*WITH_MODULATED_DCN=False"):
        _dry_load(md, mr.config(modulated=False))      # 27 channels under a dconv config
    with pytest.raises(ValueError, match=r"layer2\.0\.conv2\.offset\.weight.*WITH_MODULATED_DCN=True"):
        _dry_load(d1, mr.config(modulated=True))       # and 18 under an mdconv one
    with pytest.raises(ValueError, match=r"layer2\.0\.conv2\.offset\.weight.*STAGE_WITH_DCN.*plain"):
        _dry_load(md, MaskRCNNConfig())                # deformable weights, plain config
    with pytest.raises(ValueError, match=r"layer2\.0\.conv2\.weight.*STAGE_WITH_DCN.*deformable"):
        _dry_load(plain, mr.config())                  # plain weights, deformable config
    with pytest.raises(ValueError, match=r"layer3\.0\.conv2\.offset\.weight.*STAGE_WITH_DCN.*plain"):
        _dry_load(md, mr.config(stage_with_dcn=(False, True, False, True)))   # a deformable weight in a stage the config says is plain
    with pytest.raises(ValueError, match=r"layer1\.0\.conv2\.weight.*STAGE_WITH_DCN.*deformable"):
        _dry_load(md, mr.config(stage_with_dcn=(True, True, True, True)))     # and the reverse
    bad = dict(md); bad["backbone.body.layer4.1.conv2.conv.weight"] = np.zeros((512, 256, 3, 3), np.float32)
    with pytest.raises(ValueError, match=r"layer4\.1\.conv2\.conv\.weight.*\(512, 512, 3, 3\)"):
        _dry_load(bad, mr.config())
    bad = dict(md); del bad["backbone.body.layer4.1.conv2.offset.bias"]
    with pytest.raises(ValueError, match=r"layer4\.1\.conv2\.offset\.bias is missing"):
        _dry_load(bad, mr.config())
