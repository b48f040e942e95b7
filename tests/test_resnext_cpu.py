"""ResNeXt without a GPU: the three X-101-32x8d yamls and the config keys behind them, every refusal by its yaml key, the state-dict generators, and the
model classes' checks that run before an engine exists."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import ROOT


def _node(name=None, *opts):
    from isegmi.config import cfg
    c = cfg.clone()
    if name:
        c.merge_from_file(os.path.join(ROOT, "configs", name))
    c.merge_from_list(list(opts))
    return c


X101 = ("MODEL.BACKBONE.CONV_BODY", "R-101-FPN", "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.STRIDE_IN_1X1", False)


def test_defaults_carry_the_four_resnets_keys():
    from isegmi.config import cfg
    rn = cfg.MODEL.RESNETS
    assert (rn.NUM_GROUPS, rn.WIDTH_PER_GROUP, rn.RES2_OUT_CHANNELS, rn.STEM_OUT_CHANNELS) == (1, 64, 256, 64)


@pytest.mark.parametrize("name,mask_on", [("e2e_mask_rcnn_X_101_32x8d_FPN_1x.yaml", True), ("e2e_faster_rcnn_X_101_32x8d_FPN_1x.yaml", False)])
def test_two_stage_x101_yamls(name, mask_on):
    from isegmi.config import to_maskrcnn_config
    from isegmi.maskrcnn import MaskRCNNConfig
    text = open(os.path.join(ROOT, "configs", name)).read()
    assert "MASK_ON: %s" % mask_on in text and 'CONV_BODY: "R-101-FPN"' in text
    mc = to_maskrcnn_config(_node(name))
    want = dataclasses.replace(MaskRCNNConfig(), depth=101, CONV_BODY="R-101-FPN", NUM_GROUPS=32, WIDTH_PER_GROUP=8, STRIDE_IN_1X1=False, MASK_ON=mask_on)
    assert mc == want
    assert not mc.USE_GN and not mc.KEYPOINT_ON


def test_retinanet_x101_yaml():
    from isegmi.config import to_retinanet_config
    from isegmi.retinanet import RetinaNetConfig
    rc = to_retinanet_config(_node("retinanet_X_101_32x8d_FPN_1x.yaml"))
    assert rc == dataclasses.replace(RetinaNetConfig(), depth=101, CONV_BODY="R-101-FPN-RETINANET", NUM_GROUPS=32, WIDTH_PER_GROUP=8, STRIDE_IN_1X1=False)


def test_num_groups_1_configs_are_todays_objects():
    from isegmi.config import to_keypointrcnn_config, to_maskrcnn_config, to_retinanet_config
    from isegmi.maskrcnn import MaskRCNNConfig
    from isegmi.retinanet import RetinaNetConfig
    assert to_maskrcnn_config(_node()) == MaskRCNNConfig()
    assert to_maskrcnn_config(_node("e2e_mask_rcnn_R_50_FPN_1x.yaml")) == MaskRCNNConfig()
    assert to_maskrcnn_config(_node("e2e_faster_rcnn_R_101_FPN_1x.yaml")) == dataclasses.replace(MaskRCNNConfig(), depth=101, CONV_BODY="R-101-FPN", MASK_ON=False)
    gn = to_maskrcnn_config(_node("e2e_mask_rcnn_R_50_FPN_1x_gn.yaml"))
    assert gn.USE_GN and gn.NUM_GROUPS == 1 and gn.WIDTH_PER_GROUP == 64 and not gn.STRIDE_IN_1X1
    assert to_retinanet_config(_node("retinanet_R-50-FPN_1x.yaml")) == RetinaNetConfig()
    kp = to_keypointrcnn_config(_node("e2e_keypoint_rcnn_R_50_FPN_1x.yaml"))
    assert kp.KEYPOINT_ON and kp.NUM_GROUPS == 1
    assert to_maskrcnn_config(_node("e2e_mask_rcnn_R_50_C4_1x.yaml")).NUM_GROUPS == 1


def test_either_stride_placement_is_accepted_with_groups():
    from isegmi.config import to_maskrcnn_config, to_retinanet_config
    for v in (True, False):
        assert to_maskrcnn_config(_node(None, *X101[:6], "MODEL.RESNETS.STRIDE_IN_1X1", v)).STRIDE_IN_1X1 is v
        assert to_maskrcnn_config(_node(None, *X101[:6], "MODEL.RESNETS.STRIDE_IN_1X1", v, "MODEL.MASK_ON", False)).STRIDE_IN_1X1 is v
        assert to_retinanet_config(_node("retinanet_X_101_32x8d_FPN_1x.yaml", "MODEL.RESNETS.STRIDE_IN_1X1", v)).STRIDE_IN_1X1 is v
    assert to_maskrcnn_config(_node(None, "MODEL.RESNETS.NUM_GROUPS", 8, "MODEL.RESNETS.WIDTH_PER_GROUP", 8)).NUM_GROUPS == 8   # 64-wide: a multiple of 64


REFUSED = [
    (("MODEL.RESNETS.STRIDE_IN_1X1", False), "STRIDE_IN_1X1"),                                      # unchanged: groups 1, no GroupNorm
    (("MODEL.RESNETS.RES2_OUT_CHANNELS", 128), "RES2_OUT_CHANNELS"),
    (("MODEL.RESNETS.STEM_OUT_CHANNELS", 32), "STEM_OUT_CHANNELS"),
    (("MODEL.RESNETS.NUM_GROUPS", 0), "NUM_GROUPS"),
    (("MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 4), "WIDTH_PER_GROUP"),     # 4 channels per group in res2
    (("MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 16), "WIDTH_PER_GROUP"),    # 128 per group in res5
    (("MODEL.RESNETS.NUM_GROUPS", 4, "MODEL.RESNETS.WIDTH_PER_GROUP", 8), "NUM_GROUPS"),           # width 32: not a multiple of 64
    (("MODEL.RESNETS.WIDTH_PER_GROUP", 32), "WIDTH_PER_GROUP"),                                      # a narrow plain ResNet
    (X101 + ("MODEL.BACKBONE.CONV_BODY", "R-50-C4"), "NUM_GROUPS"),
]


@pytest.mark.parametrize("opts,key", REFUSED)
def test_two_stage_refusals_name_their_key(opts, key):
    from isegmi.config import to_maskrcnn_config
    with pytest.raises(ValueError, match=key):
        to_maskrcnn_config(_node(None, *opts))
    with pytest.raises(ValueError, match=key):
        to_maskrcnn_config(_node(None, *opts, "MODEL.MASK_ON", False))


def test_groups_with_groupnorm_keypoints_or_retinanet_misuse_raise():
    from isegmi.config import to_keypointrcnn_config, to_maskrcnn_config, to_retinanet_config
    with pytest.raises(ValueError, match="NUM_GROUPS.*GroupNorm"):
        to_maskrcnn_config(_node("e2e_mask_rcnn_R_50_FPN_1x_gn.yaml", "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8))
    with pytest.raises(ValueError, match="NUM_GROUPS.*KEYPOINT_ON"):
        to_keypointrcnn_config(_node("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8))
    with pytest.raises(ValueError, match="STRIDE_IN_1X1"):
        to_retinanet_config(_node("retinanet_R-50-FPN_1x.yaml", "MODEL.RESNETS.STRIDE_IN_1X1", False))
    for opts, key in ((("MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 16), "WIDTH_PER_GROUP"), (("MODEL.RESNETS.RES2_OUT_CHANNELS", 64), "RES2_OUT_CHANNELS"),
                      (("MODEL.RESNETS.STEM_OUT_CHANNELS", 128), "STEM_OUT_CHANNELS")):
        with pytest.raises(ValueError, match=key):
            to_retinanet_config(_node("retinanet_R-50-FPN_1x.yaml", *opts))


def test_model_classes_refuse_before_an_engine_exists():
    """fp16, the C4 body, GroupNorm and the keypoint head next to NUM_GROUPS > 1: ValueError naming the key, no device needed."""
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.retinanet import RetinaNet, RetinaNetConfig
    x = dict(NUM_GROUPS=32, WIDTH_PER_GROUP=8)
    with pytest.raises(ValueError, match="NUM_GROUPS.*fp16"):
        MaskRCNN({}, 128, 160, cfg=MaskRCNNConfig(**x), fp16=True)
    with pytest.raises(ValueError, match="NUM_GROUPS.*C4"):
        MaskRCNN({}, 128, 160, cfg=dataclasses.replace(MaskRCNNConfig.c4(), **x))
    with pytest.raises(ValueError, match="NUM_GROUPS.*GroupNorm"):
        MaskRCNN({}, 128, 160, cfg=MaskRCNNConfig(USE_GN=True, **x))
    with pytest.raises(ValueError, match="NUM_GROUPS.*KEYPOINT_ON"):
        MaskRCNN({}, 128, 160, cfg=MaskRCNNConfig(KEYPOINT_ON=True, MASK_ON=False, **x))
    with pytest.raises(ValueError, match="WIDTH_PER_GROUP"):
        MaskRCNN({}, 128, 160, cfg=MaskRCNNConfig(NUM_GROUPS=32, WIDTH_PER_GROUP=4))
    with pytest.raises(ValueError, match="WIDTH_PER_GROUP"):
        RetinaNet({}, 128, 160, cfg=RetinaNetConfig(NUM_GROUPS=32, WIDTH_PER_GROUP=16))
    with pytest.raises(ValueError, match="fp16"):
        RetinaNet({}, 128, 160, cfg=RetinaNetConfig(**x), fp16=True)


def test_resnext_state_dict_shapes():
    from isegmi.weights import maskrcnn_state_dict, retinanet_state_dict
    for sd in (maskrcnn_state_dict(3, 50, groups=32, width_per_group=8), retinanet_state_dict(3, 50, groups=32, width_per_group=8)):
        inpl = 64
        for li, nb in enumerate((3, 4, 6, 3)):
            width, out = 256 << li, 256 << li
            for b in range(nb):
                nm = "backbone.body.layer%d.%d" % (li + 1, b)
                assert sd[nm + ".conv1.weight"].shape == (width, inpl, 1, 1)
                assert sd[nm + ".conv2.weight"].shape == (width, 8 << li, 3, 3)
                assert sd[nm + ".conv3.weight"].shape == (out, width, 1, 1)
                assert sd[nm + ".bn2.weight"].shape == (width,) and sd[nm + ".bn3.weight"].shape == (out,)
                assert (nm + ".downsample.0.weight" in sd) == (b == 0)
                inpl = out
        assert sd["backbone.body.layer1.0.downsample.0.weight"].shape == (256, 64, 1, 1)
    with pytest.raises(ValueError, match="gn"):
        maskrcnn_state_dict(3, 50, gn=True, groups=32, width_per_group=8)


def test_default_arguments_reproduce_the_resnet_dicts_bit_for_bit():
    """The generators' draw order is untouched: the digest of the default dicts is the recorded one, and explicit (1, 64) equals the default."""
    import fasterrcnn_cases as fc
    from isegmi.weights import maskrcnn_state_dict, random_maskrcnn_state_dict, retinanet_state_dict
    from isegmi.maskrcnn import MaskRCNNConfig
    a, b = maskrcnn_state_dict(1234), maskrcnn_state_dict(1234, groups=1, width_per_group=64)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert fc.digest(a) == fc.digest(random_maskrcnn_state_dict(MaskRCNNConfig(), 1234))
    r, s = retinanet_state_dict(1234), retinanet_state_dict(1234, groups=1, width_per_group=64)
    assert sorted(r) == sorted(s) and all(np.array_equal(r[k], s[k]) for k in r)
    assert a["backbone.body.layer2.0.conv2.weight"].shape == (128, 128, 3, 3)
    # the trunk of the default dict, drawn by hand the way the generator did before it knew about groups
    rng = np.random.default_rng(1234)
    w = (rng.standard_normal((64, 3, 7, 7)) * np.sqrt(2.0 / (3 * 49))).astype(np.float32)
    assert np.array_equal(a["backbone.body.stem.conv1.weight"], w)
    for _ in range(4):
        rng.uniform(0.5, 1.5, 64) if _ in (0, 3) else rng.standard_normal(64)
    w1 = (rng.standard_normal((64, 64, 1, 1)) * np.sqrt(2.0 / 64)).astype(np.float32)
    assert np.array_equal(a["backbone.body.layer1.0.conv1.weight"], w1)


def test_import_tool_knows_the_x101_families():
    import importlib.util
    spec = importlib.util.spec_from_file_location("import_pth", os.path.join(ROOT, "tools", "import_pth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for fam in ("maskrcnn_x101_fpn", "fasterrcnn_x101_fpn", "retinanet_x101_fpn"):
        assert fam in mod.FAMILIES
