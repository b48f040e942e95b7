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


def third_image():
    """A third image for the small canvas (256 x 352), smaller than both of small_images()."""
    return np.random.default_rng(20261019).uniform(0, 255, (231, 322, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def three():
    """small_images() + third_image() as one batch on the small canvas, and the reference forward of the third image alone on that canvas (the layers treat
    the images of a batch independently: images 0 and 1 are reference("small")'s).  -> (x [3], hw [3], ref of image 2, dets of image 2)"""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images(small_images() + [third_image()])
    ref = rr.RetinaNetRef(state_dict(), cap=128)
    dets = ref.forward(x[2:3], hw[2:3])
    x.setflags(write=False)
    return x, hw, ref, dets


def state_dict_convs(num_convs):
    """state_dict() with the towers cut to their first num_convs layers."""
    drop = tuple("rpn.head.%s_tower.%d." % (t, 2 * i) for t in ("cls", "bbox") for i in range(num_convs, 4))
    return {k: v for k, v in state_dict().items() if not k.startswith(drop)}


@functools.lru_cache(maxsize=None)
def heads(which, num_convs):
    """(logits, deltas) of reference(which)'s pyramid under towers of num_convs layers: the trunk and the pyramid are not computed again."""
    ref = reference(which, cap=128)[2]
    return rr.RetinaNetRef(state_dict(), num_convs=num_convs).heads(ref.feats["P"])


def tail(which, num_convs=4, **kw):
    """rr.tail on reference(which)'s head outputs (or heads(which, num_convs)'s) with other tail parameters (top_n, thr, nms_thr, det_per_img, ...).
    -> (sel[l][n], dets)"""
    x, hw, ref, _ = reference(which, cap=128)
    logits, deltas = (ref.feats["logits"], ref.feats["deltas"]) if num_convs == 4 else heads(which, num_convs)
    sel, dec, dets, totals = rr.tail(logits, deltas, ref.feats["anchors"], hw, **dict(ref.kw, **kw))
    return sel, [dict(box=d[0], score=d[1], label=d[2]) for d in dets]


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
    assert_selected_equal(model, ref.feats["sel"], n)


def assert_selected_equal(model, want, n, first=0):
    """Every level's selected list of the last forward's images first .. first + n - 1 against want[l][0 .. n - 1]."""
    sel = model.selected(first + n)
    for l in range(5):
        for i in range(n):
            s, idx = want[l][i]
            assert len(sel[l][first + i][1]) == len(idx), (l, i, len(sel[l][first + i][1]), len(idx))
            assert np.array_equal(sel[l][first + i][1], idx), (l, i)
            assert np.array_equal(bits(sel[l][first + i][0]), bits(s)), (l, i)
