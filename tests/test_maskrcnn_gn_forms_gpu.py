"""The GroupNorm Mask R-CNN engine in every form it launches GroupNorm in (tests/test_fallback_paths_gpu.py checks the same forms for the FrozenBN weights
only): resnet_stage's three ways to run a projection block's norms -- behind the grouped conv1 + projection launch (default), on a side stream with its
own gn.ws:<layer> and a join before conv3 (`conv_groups` 0), plainly in order (`multi_stream` 0) -- the grouped and per-level FPN, the RPN selection
forms, aliased and per-layer trunk buffers (GroupNorm runs in place on them); a short batch; a canvas change, eager and under hipGraph; and group
configurations other than 32 groups at eps 1e-5.  fp32, the seeded weights and the small canvas of tests/test_maskrcnn_gn_gpu.py, bit for bit against
tests/maskrcnn_gn_ref.py.  Every run does two forwards and a paste, and the second must equal the first."""
import ctypes as C
import os

import numpy as np
import pytest

import maskrcnn_gn_common as M
from maskrcnn_gn_common import sd, small  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GN_YAML = os.path.join(ROOT, "configs", "e2e_mask_rcnn_R_50_FPN_1x_gn.yaml")

VARIANTS = [dict(conv_groups=0), dict(conv_groups=0, multi_stream=0), dict(multi_stream=0), dict(alias_buffers=0), dict(alias_buffers=0, conv_groups=0),
            dict(rpn_select_groups=0), dict(rpn_select_groups=2), dict(conv_groups=1, rpn_select_groups=0),
            dict(conv_groups=0, rpn_select_groups=0, rpn_select_on_tail=0)]


def _model(sd, H, W, cfg, max_batch, params=()):
    from isegmi.maskrcnn import MaskRCNN
    model = MaskRCNN(sd, H, W, cfg=cfg, max_batch=max_batch)
    for k, v in dict(params).items():
        model.set_param(k, float(v))
    return model


def _run_twice(sd, x, hw, cfg, params):
    model = _model(sd, x.shape[1], x.shape[2], cfg, x.shape[0], params)
    first = M.forward_and_fetch(model, x, hw)
    second = M.forward_and_fetch(model, x, hw)   # runs against the first one's tail (WAR fences, side-stream joins, reused gn.ws:* workspaces)
    model.close()
    M.assert_same(second, first, "second forward, %r" % (params,))
    return first


def _graph_stats(model):
    cap, rep, fail = C.c_int64(), C.c_int64(), C.c_int64()
    from isegmi import _ffi
    _ffi.check(_ffi.lib().isegmi_engine_graph_stats(model._h, C.byref(cap), C.byref(rep), C.byref(fail)))
    return cap.value, rep.value, fail.value


@pytest.mark.parametrize("N", [2, 1])
def test_gn_launch_forms_are_bit_identical(ffi, sd, small, N):
    x, hw, ref, rd = small
    x, hw, rd = x[:N], hw[:N], rd[:N]   # image 0 alone pads to the same canvas, and the reference is per image
    assert x.shape == (N, 256, 352, 3)
    base = _run_twice(sd, x, hw, M.gn_cfg(), {})
    M.assert_equals_reference(base, {k: ref.feats[k][:N] for k in M.LEVELS}, rd, (256, 352), "default")
    for v in VARIANTS:
        M.assert_same(_run_twice(sd, x, hw, M.gn_cfg(), v), base, "variant %r" % (v,))


def test_gn_short_batch_in_a_batch_of_two_engine(ffi, sd, small):
    """max_batch = 2: the batch, image 0 alone (every GroupNorm launch and gn.ws:* sized for two images runs over one), the batch again."""
    from isegmi.maskrcnn import prepare_images
    x, hw, ref, rd = small
    x1, hw1 = prepare_images(M.small_images()[:1])
    assert x1.shape == (1, 256, 352, 3) and np.array_equal(x1[0], x[0])
    model = _model(sd, 256, 352, M.gn_cfg(), 2)
    feats = {k: ref.feats[k] for k in M.LEVELS}
    before = M.forward_and_fetch(model, x, hw)
    M.assert_equals_reference(before, feats, rd, (256, 352), "batch of two")
    alone = M.forward_and_fetch(model, x1, hw1)
    M.assert_equals_reference(alone, {k: v[:1] for k, v in feats.items()}, rd[:1], (256, 352), "image 0 alone")
    M.assert_same(M.forward_and_fetch(model, x, hw), before, "batch of two, after the short batch")
    model.close()


def test_gn_canvas_change_eager_and_graph(ffi, sd):
    """An engine built for 256 x 352 serves that canvas (two images), then 128 x 160 (one image: every activation and gn.ws:* buffer was sized by the
    larger shape and is reused by the smaller), then the large one again; then the same under hipGraph, whose graphs are per canvas."""
    xb, hwb, refb, rdb = M.reference_few("small")
    xs, hws, refs, rds = M.reference_few("tiny")
    assert xb.shape == (2, 256, 352, 3) and xs.shape == (1, 128, 160, 3)
    assert min(len(r["score"]) for r in rdb) >= 3 and len(rds[0]["proposals"]) > 20
    model = _model(sd, 256, 352, M.few(), 2)
    big = M.forward_and_fetch(model, xb, hwb)
    M.assert_equals_reference(big, refb.feats, rdb, (256, 352), "large canvas")
    tiny = M.forward_and_fetch(model, xs, hws)
    M.assert_equals_reference(tiny, refs.feats, rds, (128, 160), "small canvas after the large one")
    M.assert_same(M.forward_and_fetch(model, xb, hwb), big, "large canvas after the small one")
    big_o = {k: v for k, v in big.items() if k not in M.LEVELS + ("box.xconv3",)}
    tiny_o = {k: v for k, v in tiny.items() if k not in M.LEVELS + ("box.xconv3",)}
    model.set_param("graph", 1.0)
    replays = []
    for name, x, hw, want in (("big", xb, hwb, big_o), ("big", xb, hwb, big_o), ("tiny", xs, hws, tiny_o), ("tiny", xs, hws, tiny_o), ("big", xb, hwb, big_o)):
        M.assert_same(M.forward_and_fetch(model, x, hw, features=False), want, "graph = 1, %s, step %d" % (name, len(replays)))
        cap, rep, fail = _graph_stats(model)
        assert fail == 0, (cap, rep, fail)
        replays.append(rep)
    assert replays[1] > replays[0] and replays[3] > replays[2], replays   # each canvas was replayed from its graph at least once
    model.close()


def _yaml_cfg(*opts):
    from isegmi.config import cfg, to_maskrcnn_config
    c = cfg.clone()
    c.merge_from_file(GN_YAML)
    c.merge_from_list(list(opts) + ["MODEL.RPN.POST_NMS_TOP_N_TEST", M.FEW, "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", M.FEW])
    return to_maskrcnn_config(c)


GROUP_CONFIGS = {
    # 8 channels per group everywhere: 8 groups at the stem, 256 at res5's output; and an eps the kernels never ran with
    "dim_per_gp_8_eps_1e-3": (dict(GN_DIM_PER_GP=8, GN_NUM_GROUPS=32, GN_EPSILON=1e-3),
                              ("MODEL.GROUP_NORM.DIM_PER_GP", 8, "MODEL.GROUP_NORM.NUM_GROUPS", -1, "MODEL.GROUP_NORM.EPSILON", 1e-3),
                              dict(dim_per_gp=8, eps=1e-3)),
    # 64 groups: one channel per group in the 64-channel layers (a float4 holds four groups)
    "num_groups_64": (dict(GN_NUM_GROUPS=64), ("MODEL.GROUP_NORM.NUM_GROUPS", 64), dict(num_groups=64)),
}


@pytest.mark.parametrize("name", sorted(GROUP_CONFIGS))
def test_gn_group_configurations(ffi, sd, name):
    """One image, 200 proposals; the configuration built from the yaml with overrides and as a MaskRCNNConfig directly: the same object, and the engine
    equals the reference run with the same groups / eps.  (tests/test_groupnorm_cpu.py checks that each configuration still yields detections.)"""
    fields, opts, ref_kw = GROUP_CONFIGS[name]
    cfg = M.few(**fields)
    from_yaml = _yaml_cfg(*opts)
    assert (from_yaml.GN_NUM_GROUPS, from_yaml.GN_DIM_PER_GP, from_yaml.GN_EPSILON) == (cfg.GN_NUM_GROUPS, cfg.GN_DIM_PER_GP, cfg.GN_EPSILON)
    assert from_yaml.USE_GN and from_yaml.RPN_POST_NMS_TOP_N_TEST == M.FEW == from_yaml.RPN_FPN_POST_NMS_TOP_N_TEST
    x, hw, ref, rd = M.reference_few("first", **ref_kw)
    assert len(rd[0]["score"]) >= 3
    results = []
    for c in (cfg, from_yaml):
        got = _run_twice(sd, x, hw, c, {})
        M.assert_equals_reference(got, ref.feats, rd, (256, 352), name)
        results.append(got)
    M.assert_same(results[1], results[0], "yaml against dataclass")
