"""Reference of test-time box augmentation (TEST.BBOX_AUG) in numpy fp32, in the operators' stated order (TEST INFRASTRUCTURE ONLY):
the per-view candidate stage (isegmi_op_bbox_aug_candidates), the pool with its cap, and the merge.  Built on the restatements the tests already have:
the oracle's softmax and box decode (oracle/ora.py) and retinanet_ref.postprocess (class-wise NMS + the detection cut over candidate lists).

The three `wrong` switches restate a rule the WRONG way; tests/test_bbox_aug_cpu.py shows that the crafted cases tell each of them from the right one."""
import numpy as np

import retinanet_ref as rr
from oracle import ora

F32 = np.float32
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def unflip(boxes, w_view, drop_minus_one=False):
    """BoxList.transpose(FLIP_LEFT_RIGHT) with TO_REMOVE = 1, two fp32 subtractions per coordinate: x1' = (w - x2) - 1, x2' = (w - x1) - 1."""
    b = np.array(boxes, F32).reshape(-1, 4)
    w, one = F32(w_view), F32(0.0 if drop_minus_one else 1.0)
    x1 = (w - b[:, 2]) - one
    x2 = (w - b[:, 0]) - one
    b[:, 0], b[:, 2] = x1, x2
    return b


def to_view0(boxes, ratios_wh):
    """BoxList.resize: one fp32 multiplication per coordinate"""
    rw, rh = F32(ratios_wh[0]), F32(ratios_wh[1])
    return np.asarray(boxes, F32).reshape(-1, 4) * np.array([rw, rh, rw, rh], F32)


def view_ratios(hw0, hw_view):
    """(w0 / w_view, h0 / h_view) as float32 of the double quotient (BoxList.resize, MaskRCNN._resize_ratios)"""
    return F32(float(hw0[1]) / float(hw_view[1])), F32(float(hw0[0]) / float(hw_view[0]))


def clip(boxes, w, h):
    b = np.array(boxes, F32).reshape(-1, 4)
    mx, my = F32(w) - F32(1.0), F32(h) - F32(1.0)
    for k, hi in ((0, mx), (1, my), (2, mx), (3, my)):
        v = b[:, k]
        b[:, k] = np.where(v < 0, F32(0.0), np.where(v > hi, hi, v))
    return b


def candidates(logits, regr, props, prop_cnt, image_hw, hflip=False, ratios_wh=(1.0, 1.0), thr=0.05, cls_agnostic=False, wrong=None):
    """One image of one view.  logits [R, ncls], regr [R, 4 * ncls] (cls_agnostic: [R, 8]), props [R, 4]; only rows below prop_cnt are looked at.
    -> (boxes [M, 4] in view-0 coordinates, scores [M], labels [M]) in (proposal asc, class asc) order.
    wrong: None, "no_minus_one" (the flip drops TO_REMOVE), "flip_before_clip" (unflip, then clip: the mirror map x -> (w - x) - 1 is monotone and maps
    the clip range [0, w - 1] onto itself, so this one changes NO answer -- the tests assert that), "clip_last" (unflip, rescale, then clip against the
    view's size: the order that does matter) or "ge" (p >= thr)."""
    n = int(prop_cnt)
    logits = np.asarray(logits, F32)[:n]; regr = np.asarray(regr, F32)[:n]; props = np.asarray(props, F32)[:n]
    ncls = logits.shape[1]
    h, w = int(image_hw[0]), int(image_hw[1])
    if n == 0:
        return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    p = ora.softmax(logits)
    ok = (p >= F32(thr)) if wrong == "ge" else (p > F32(thr))
    ok[:, 0] = False
    rows, labels = np.nonzero(ok)   # row-major: proposal ascending, class ascending inside a proposal
    cols = 4 + np.arange(4)[None, :] if cls_agnostic else 4 * labels[:, None] + np.arange(4)[None, :]
    d = np.ascontiguousarray(regr[rows[:, None], cols])
    pr = np.ascontiguousarray(props[rows])
    if wrong in ("flip_before_clip", "clip_last"):
        b = ora.decode_boxes(pr, d, WEIGHTS, float(w), float(h), clip=False) if len(rows) else np.zeros((0, 4), F32)
        b = unflip(b, w) if hflip else b
        if wrong == "clip_last":   # the clip in view-0 coordinates against the VIEW's size
            return clip(to_view0(b, ratios_wh), w, h), p[rows, labels].astype(F32), labels.astype(np.int32)
        b = clip(b, w, h)
    else:
        b = ora.decode_boxes(pr, d, WEIGHTS, float(w), float(h), clip=True) if len(rows) else np.zeros((0, 4), F32)
        if hflip:
            b = unflip(b, w, drop_minus_one=(wrong == "no_minus_one"))
    return to_view0(b, ratios_wh), p[rows, labels].astype(F32), labels.astype(np.int32)


def pool(views, cap=8192, entry=None):
    """Concatenates the views' candidate lists of one image, view-major.  entry: (boxes, scores, labels) already in the pool.
    -> (boxes, scores, labels) of the first `cap`, total (uncapped)."""
    parts = ([entry] if entry is not None else []) + list(views)
    b = np.concatenate([np.asarray(v[0], F32).reshape(-1, 4) for v in parts]) if parts else np.zeros((0, 4), F32)
    s = np.concatenate([np.asarray(v[1], F32) for v in parts]) if parts else np.zeros(0, F32)
    lb = np.concatenate([np.asarray(v[2], np.int32) for v in parts]) if parts else np.zeros(0, np.int32)
    return (b[:cap], s[:cap], lb[:cap]), len(s)


def merge(pooled, ncls, nms_thr=0.5, det_per_img=100, cap=100, nms_flags=0):
    """filter_results' second half over the pool: per class greedy NMS in (score desc, slot asc) order, class order, the kth-value cut."""
    return rr.postprocess(pooled[0], pooled[1], pooled[2], nms_thr, det_per_img, cap, nms_flags, ncls=ncls)


def detect(views, ncls, thr=0.05, nms_thr=0.5, det_per_img=100, cap=100, nms_flags=0, pool_cap=8192, cls_agnostic=False, wrong=None):
    """views: list of dict(logits, regr, props, prop_cnt, image_hw, hflip, ratios_wh) of ONE image, view 0 first.
    -> ((boxes, scores, labels), pool total, per-view candidate counts)"""
    cands = [candidates(v["logits"], v["regr"], v["props"], v["prop_cnt"], v["image_hw"], v.get("hflip", False), v.get("ratios_wh", (1.0, 1.0)), thr,
                        cls_agnostic, wrong) for v in views]
    pooled, total = pool(cands, pool_cap)
    return merge(pooled, ncls, nms_thr, det_per_img, cap, nms_flags), total, [len(c[1]) for c in cands]
