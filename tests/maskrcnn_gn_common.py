"""What the GroupNorm Mask R-CNN engine tests share (TEST INFRASTRUCTURE ONLY; tests/test_maskrcnn_gn_gpu.py, tests/test_maskrcnn_gn_forms_gpu.py and the
reference-only checks of tests/test_groupnorm_cpu.py): the seeded weights, the small canvas with its reference forward -- computed once per process,
never modified -- and the comparison helpers.  The test modules import the fixtures `sd` and `small` from here."""
import dataclasses
import functools

import numpy as np
import pytest

from maskrcnn_gn_ref import MaskRCNNGNRef  # noqa: F401  (re-exported)

SEED = 1234
FEW = 200   # proposals per image where a test pays for its own reference forward


def gn_cfg(**kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return dataclasses.replace(MaskRCNNConfig(), USE_GN=True, STRIDE_IN_1X1=False, BOX_HEAD="FPNXconv1fcFeatureExtractor", **kw)


def few(**kw):
    """gn_cfg with FEW proposals per level and per image: keeps a CPU reference forward at a few seconds."""
    return gn_cfg(RPN_POST_NMS_TOP_N_TEST=FEW, RPN_FPN_POST_NMS_TOP_N_TEST=FEW, **kw)


@functools.lru_cache(maxsize=None)
def state_dict():
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(SEED, gn=True)


def small_images():
    rng = np.random.default_rng(20261003)
    return [rng.uniform(0, 255, (250, 340, 3)).astype(np.float32), rng.uniform(0, 255, (256, 300, 3)).astype(np.float32)]


def tiny_image():
    """One 100 x 130 image: canvas 128 x 160, smaller than the small canvas in both directions."""
    return [np.random.default_rng(20261018).uniform(0, 255, (100, 130, 3)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def small_reference():
    """The small canvas of tests/test_maskrcnn_e2e_gpu.py, bs = 2, and its reference forward at the default 1000 proposals."""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images(small_images())
    ref = MaskRCNNGNRef(state_dict())
    rd = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, rd


@functools.lru_cache(maxsize=None)
def reference_few(which, **gn_kw):
    """Reference forward at FEW proposals of "small" (the two images), "first" (image 0 alone: the same canvas) or "tiny"; gn_kw: num_groups /
    dim_per_gp / eps of MaskRCNNGNRef.  -> (x, hw, ref, rd)"""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images({"small": small_images, "first": lambda: small_images()[:1], "tiny": tiny_image}[which]())
    ref = MaskRCNNGNRef(state_dict(), post_nms=FEW, fpn_post=FEW, **gn_kw)
    rd = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, rd


@pytest.fixture(scope="module")
def sd():
    return state_dict()


@pytest.fixture(scope="module")
def small():
    return small_reference()


KEYS = ("proposal_count", "proposals", "proposal_scores", "det.count", "det.box", "det.score", "det.label", "det.mask28", "det.masks")
LEVELS = ("P2", "P3", "P4", "P5", "P6")


def forward_and_fetch(model, x, hw, features=True):
    """One forward + paste on the batch's own canvas -> every output of KEYS trimmed to what is defined (rows below the counts), the FPN levels and the
    box head's last GroupNorm output (rows of real proposals).  `features` False (under graph replay the engine does not revisit its buffers' shapes)
    leaves the last two out."""
    n = x.shape[0]
    model.upload(x, hw); model.forward_device(n); model.paste_device(x.shape[1], x.shape[2]); model.sync()
    raw = {k: model.fetch(k, n) for k in KEYS}
    pc, dc = raw["proposal_count"], raw["det.count"]
    out = {"proposal_count": pc.copy(), "det.count": dc.copy()}
    for k in ("proposals", "proposal_scores"):
        out[k] = [raw[k][i, : pc[i]] for i in range(n)]
    for k in ("det.box", "det.score", "det.label", "det.mask28", "det.masks"):
        out[k] = [raw[k][i, : dc[i]] for i in range(n)]
    if features:
        for k in LEVELS:
            out[k] = model.fetch(k, n)
        R = int(model.cfg.RPN_FPN_POST_NMS_TOP_N_TEST)
        xf = model.fetch("box.xconv3", n * R).reshape(n, R, 7, 7, -1)
        out["box.xconv3"] = [xf[i, : pc[i]] for i in range(n)]
    return out


def assert_same(a, b, what=""):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]), (what, k)
            for i, (u, v) in enumerate(zip(a[k], b[k])):
                assert u.shape == v.shape and np.array_equal(u, v), (what, k, i)
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def assert_equals_reference(got, feats, rd, canvas, what=""):
    """Engine outputs (forward_and_fetch) against a MaskRCNNGNRef forward (its .feats and per-image results), bit for bit: FPN levels, proposals, the box head's features, detections, 28 x 28
    masks and the pasted masks."""
    for k in LEVELS:
        if k in got:
            assert got[k].shape == feats[k].shape and np.array_equal(got[k], feats[k]), (what, k)
    for i, r in enumerate(rd):
        assert got["proposal_count"][i] == len(r["proposals"]), (what, i)
        assert np.array_equal(got["proposals"][i], r["proposals"]) and np.array_equal(got["proposal_scores"][i], r["proposal_scores"]), (what, i)
        if "box.xconv3" in got:
            assert np.array_equal(got["box.xconv3"][i], r["xconv"]), (what, i)
        assert got["det.count"][i] == len(r["score"]), (what, i)
        assert np.array_equal(got["det.label"][i].astype(np.int64), r["label"].astype(np.int64)), (what, i)
        assert np.array_equal(got["det.score"][i], r["score"]) and np.array_equal(got["det.box"][i], r["box"]), (what, i)
        assert np.array_equal(got["det.mask28"][i], r["mask28"]), (what, i)
        rm, _ = MaskRCNNGNRef.paste(r, canvas[0], canvas[1])
        assert np.array_equal(got["det.masks"][i][: len(rm)], rm), (what, i)
