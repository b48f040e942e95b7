"""What the RetinaNet engine tests share (TEST INFRASTRUCTURE ONLY): the seeded weights and the reference forwards, computed once per process and never
modified."""
import functools

import numpy as np

import retinanet_ref as rr
from maskrcnn_gn_common import small_images, tiny_image

SEED = 1234
LEVELS = ("P3", "P4", "P5", "P6", "P7")


@functools.lru_cache(maxsize=None)
def state_dict(depth=50):
    from isegmi.weights import retinanet_state_dict
    return retinanet_state_dict(SEED, depth)


@functools.lru_cache(maxsize=None)
def reference(which, **kw):
    """Reference forward of "small" (two images, canvas 256 x 352), "first" (image 0 alone, the same canvas) or "tiny" (one image, canvas 128 x 160);
    kw: RetinaNetRef's.  -> (x, hw, ref, dets)"""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images({"small": small_images, "first": lambda: small_images()[:1], "tiny": tiny_image}[which]())
    ref = rr.RetinaNetRef(state_dict(), **kw)
    dets = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, dets


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_dets_equal(preds, dets):
    assert len(preds) == len(dets)
    for i, (p, d) in enumerate(zip(preds, dets)):
        assert len(p) == len(d["score"]), (i, len(p), len(d["score"]))
        assert np.array_equal(p.get_field("labels"), d["label"]), i
        assert np.array_equal(bits(p.get_field("scores")), bits(d["score"])), i
        assert np.array_equal(bits(p.bbox), bits(d["box"])), i


def assert_forward_equal(model, ref, n, features=True):
    """The last forward's pyramid and every level's selected list against the reference's."""
    if features:
        for l, name in enumerate(LEVELS):
            got = model.fetch(name, n)
            assert got.shape == ref.feats["P"][l].shape, (name, got.shape)
            assert np.array_equal(bits(got), bits(ref.feats["P"][l])), name
    sel = model.selected(n)
    for l in range(5):
        for i in range(n):
            s, idx = ref.feats["sel"][l][i]
            assert np.array_equal(sel[l][i][1], idx), (l, i)
            assert np.array_equal(bits(sel[l][i][0]), bits(s)), (l, i)
