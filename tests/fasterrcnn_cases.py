"""What the Faster R-CNN tests share (TEST INFRASTRUCTURE ONLY; tests/test_fasterrcnn_cpu.py, tests/test_fasterrcnn_gpu.py,
tests/test_fasterrcnn_ops_gpu.py): the crafted class-agnostic input, the two readings of eight-wide regression rows, the box-only block formula,
and the small canvases with their oracle forward -- computed once per process, never modified."""
import functools
import hashlib

import numpy as np


def digest(sd):
    """sha256 over a state dict's sorted keys, dtypes, shapes and bytes."""
    h = hashlib.sha256()
    for k in sorted(sd):
        a = np.ascontiguousarray(sd[k])
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def agnostic_regr(reg8, ncls):
    """MODEL.CLS_AGNOSTIC_BBOX_REG as the per-class oracle sees it: box_regression[:, -4:] repeated for every class.  reg8 [..., 8] -> [..., 4 * ncls]"""
    return np.ascontiguousarray(np.tile(np.asarray(reg8, np.float32)[..., 4:8], ncls))


def per_class_reading(reg8, ncls):
    """The per-class addressing (class j at 4j .. 4j+3 from the row's start) applied to the SAME memory: rows eight floats apart, so class 2 of row i
    reads the first four floats of row i + 1 (zeros past the last row).  reg8 [R, 8] -> [R, 4 * ncls]"""
    reg8 = np.asarray(reg8, np.float32)
    flat = np.concatenate([reg8.reshape(-1), np.zeros(4 * ncls, np.float32)])
    return np.stack([flat[8 * i: 8 * i + 4 * ncls] for i in range(reg8.shape[0])])


def crafted():
    """Three proposals, three classes (background + 2): proposals 0 and 1 overlap heavily and both score for class 2, proposal 2 scores for class 1.
    The first four deltas of a row shift a box far to the right, the last four shrink it a little: which four a class decodes decides the boxes,
    and through their overlap what the NMS keeps.  -> dict(logits [3,3], reg8 [3,8], props [3,4], hw (h, w))"""
    props = np.array([[20, 20, 119, 99], [24, 22, 121, 103], [150, 40, 229, 159]], np.float32)
    logits = np.array([[0.0, -2.0, 3.0], [0.0, -2.0, 2.5], [0.0, 3.0, -2.0]], np.float32)
    reg8 = np.array([[8.0, 0.0, 0.0, 0.0, 0.5, -0.25, -0.2, -0.1],
                     [-6.0, 1.0, 0.5, 0.0, -0.5, 0.25, -0.1, -0.3],
                     [2.0, -3.0, 0.0, 0.7, 0.1, 0.2, -0.4, 0.3]], np.float32)
    return dict(logits=logits, reg8=reg8, props=props, hw=(200, 260), ncls=3)


def crowded(R, seed=5, ncls=4):
    """R proposals (one image) with one crowded class: class 2 scores above the threshold on every proposal (with R > 128 it is handed to the chip-wide
    suppression matrix, or takes the in-block bitmask NMS), the other classes on a few; tightly clustered boxes so the NMS really suppresses."""
    rng = np.random.default_rng(seed + R)
    c = rng.uniform(60, 500, (max(R // 6, 1), 2))
    ctr = c[rng.integers(0, c.shape[0], R)] + rng.normal(0, 6.0, (R, 2))
    wh = rng.uniform(30, 120, (R, 2))
    props = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    logits = rng.normal(0, 1.0, (R, ncls)).astype(np.float32)
    logits[:, 0] += 1.0
    logits[:, 2] += 3.0
    reg8 = np.concatenate([rng.normal(0, 3.0, (R, 4)), rng.normal(0, 0.4, (R, 4))], 1).astype(np.float32)
    return dict(logits=logits, reg8=reg8, props=props, hw=(600, 640), ncls=ncls)


def box_block_bytes(n, K):
    """Size of the box-only record block, written out from its definition: 16 status bytes, n*K boxes of 16, n counts, n*K scores, n*K labels of 4, every
    section padded to a multiple of 8."""
    r8 = lambda v: -(-v // 8) * 8
    return 16 + r8(n * K * 16) + r8(n * 4) + r8(n * K * 4) + r8(n * K * 4)


# ---- the small canvas of tests/test_maskrcnn_e2e_gpu.py (256 x 352, two images) with its oracle forward
def small_images():
    rng = np.random.default_rng(20261003)
    return [rng.uniform(0, 255, (250, 340, 3)).astype(np.float32), rng.uniform(0, 255, (256, 300, 3)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def full_state_dict():
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(1234)


@functools.lru_cache(maxsize=None)
def small_reference():
    """-> (x, hw, ref, rd): MaskRCNNRef(full dict).forward on the small canvas."""
    from isegmi.maskrcnn import prepare_images
    from oracle.maskrcnn_ref import MaskRCNNRef
    x, hw = prepare_images(small_images())
    ref = MaskRCNNRef(full_state_dict())
    rd = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, rd


def tiny_batch():
    """One 100 x 130 image: canvas 128 x 160."""
    from isegmi.maskrcnn import prepare_images
    return prepare_images([np.random.default_rng(20261018).uniform(0, 255, (100, 130, 3)).astype(np.float32)])


DET_KEYS = ("det.count", "det.box", "det.score", "det.label")


def fetch_dets(model, n):
    """det.* of the last forward, rows past each image's count cut off."""
    cnt = model.fetch("det.count", n)
    out = {"det.count": cnt.copy()}
    for k in DET_KEYS[1:]:
        a = model.fetch(k, n)
        out[k] = [a[i, : cnt[i]].copy() for i in range(n)]
    return out


def assert_same_dets(a, b, what=""):
    assert np.array_equal(a["det.count"], b["det.count"]), (what, a["det.count"], b["det.count"])
    for k in DET_KEYS[1:]:
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            assert u.shape == v.shape and np.array_equal(u, v), (what, k, i)


def count_launches(model, n):
    """Launches of one forward of the batch already uploaded, as the engine's own statistics count them: convolution launches (conv_timing pass) plus the
    launch groups of the other stages (op_timing pass)."""
    import ctypes as C
    from isegmi import _ffi
    L = _ffi.lib()
    f, ms, nconv = C.c_double(), C.c_double(), C.c_int64()
    model.set_param("conv_timing", 1.0)
    model.forward_device(n); model.sync()
    _ffi.check(L.isegmi_engine_conv_stats(model._h, C.byref(f), C.byref(ms), C.byref(nconv)))
    model.set_param("conv_timing", 0.0)
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    model.set_param("op_timing", 1.0)
    _ffi.check(L.isegmi_engine_op_stats(model._h, names, 16384, us, by, ln, cap, C.byref(cnt)))   # clear
    model.forward_device(n); model.sync()
    _ffi.check(L.isegmi_engine_op_stats(model._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    model.set_param("op_timing", 0.0)
    return int(nconv.value) + sum(int(ln[i]) for i in range(cnt.value))


def predictor_rows(model, sd, n=1):
    """The engine's own box-head intermediates of the last forward: (fc7 rows, cls_bbox rows, proposals) of image 0's real proposals, and the fused
    predictor weights of `sd` -> (f7 [R,1,1,C], cb [R,width], props [R,4], w [width,1,1,C], b [width])"""
    pc = int(model.fetch("proposal_count", n)[0])
    f7 = model.fetch("box.fc7")[:pc]
    cb = model.fetch("box.cls_bbox")[:pc].reshape(pc, -1)
    props = model.fetch("proposals", n)[0, :pc]
    w = np.concatenate([sd["roi_heads.box.predictor.cls_score.weight"], sd["roi_heads.box.predictor.bbox_pred.weight"]], 0)
    b = np.concatenate([sd["roi_heads.box.predictor.cls_score.bias"], sd["roi_heads.box.predictor.bbox_pred.bias"]])
    return f7, cb, props, w.reshape(w.shape[0], 1, 1, w.shape[1]), b
