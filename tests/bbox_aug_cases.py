"""Inputs of the test-time box augmentation tests (TEST INFRASTRUCTURE ONLY; tests/test_bbox_aug_cpu.py, tests/test_bbox_aug_ops_gpu.py): crafted views
that tell the rules of the candidate stage apart, and generated predictor outputs with a chosen pass pattern.  Built on first use, never modified."""
import functools

import numpy as np

F32 = np.float32
RATIO_23 = (F32(800.0 / 1200.0), F32(800.0 / 1200.0))


def _props(rng, R, w, h):
    c = np.stack([rng.uniform(0, w, R), rng.uniform(0, h, R)], 1)
    wh = rng.uniform(4, max(w, h) / 2, (R, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)


def pattern_logits(rng, R, ncls, pattern):
    """Logits [R, ncls] and the threshold under which `pattern` holds by a wide margin: "all" -- every class of every row passes (near-uniform rows, thr 0);
    "none" -- nothing passes (thr 1: no probability exceeds it); "alternate" -- class j of row r passes iff (r + j) is odd: the passing classes share
    about 2 / ncls each, the others sit 20 below (ncls 2: rows with odd r + 1 pass class 1)."""
    if pattern == "all":
        return rng.uniform(-0.5, 0.5, (R, ncls)).astype(F32), 0.0
    if pattern == "none":
        return rng.uniform(-2.0, 2.0, (R, ncls)).astype(F32), 1.0
    assert pattern == "alternate"
    r, j = np.meshgrid(np.arange(R), np.arange(ncls), indexing="ij")
    on = ((r + j) % 2 == 1)
    x = np.where(on, 0.0, -20.0) + rng.uniform(-0.05, 0.05, (R, ncls))
    return x.astype(F32), 0.5 / ncls   # a passing class holds >= 1 / (ncls / 2 + 1) of the row, a failing one < e^-19


@functools.lru_cache(maxsize=None)
def generated(R, ncls, pattern, agnostic, hw=(333, 500), seed=0):
    """N = 4 images with proposal counts (0, 1, R - 1, R) (R = 1: 0, 1, 0, 1); rows at or past a count are poisoned with NaN in logits, regressions and
    proposals.  -> dict(logits [4,R,ncls], regr [4,R,4*ncls | 8], props [4,R,4], cnt [4], hw [4,2], thr)"""
    rng = np.random.default_rng(1000 * R + 10 * ncls + seed)
    N = 4
    cnt = np.array([0, 1, max(R - 1, 0), R], np.int32)
    logits = np.empty((N, R, ncls), F32)
    thr = 0.0
    for n in range(N):
        logits[n], thr = pattern_logits(rng, R, ncls, pattern)
    regr = rng.normal(0, 1.5, (N, R, 8 if agnostic else 4 * ncls)).astype(F32)
    hws = np.array([hw, (hw[0] + 1, hw[1] + 1), hw, (hw[0] - 3, hw[1] - 7)], np.int32)
    props = np.stack([_props(rng, R, float(hws[n, 1]), float(hws[n, 0])) for n in range(N)])
    for n in range(N):
        logits[n, cnt[n]:] = np.nan; regr[n, cnt[n]:] = np.nan; props[n, cnt[n]:] = np.nan
    for a in (logits, regr, props, cnt, hws):
        a.setflags(write=False)
    return dict(logits=logits, regr=regr, props=props, cnt=cnt, hw=hws, thr=thr, ncls=ncls, agnostic=bool(agnostic))


def border_view(w_view, h_view=60):
    """Five proposals of one view, three classes, zero regressions except where noted, every class-1 probability far above 0.05: boxes that touch the left
    border, the right border, both, neither, and one whose decode lands outside the image on both sides (deltas that widen it) and is clipped to both."""
    w = float(w_view)
    props = np.array([[0, 5, 20, 30], [w - 21, 8, w - 1, 40], [0, 0, w - 1, h_view - 1], [10, 10, 30, 35], [w / 2 - 4, 20, w / 2 + 4, 30]], F32)
    logits = np.tile(np.array([0.0, 3.0, -6.0], F32), (5, 1))
    regr = np.zeros((5, 12), F32)
    regr[4, 4:8] = (0.0, 0.0, 25.0, 0.0)     # class 1: dw / 5 = 5 > the clamp: 62.5 times as wide
    return dict(logits=logits, regr=regr, props=props, prop_cnt=5, image_hw=(h_view, int(w_view)))


def clip_order_view():
    """One proposal whose class-1 decode overshoots the right border of a 100-wide view that is twice as small as view 0 (ratio 2): clipped in the view it
    ends at x = 99 -> 198 in view 0; clipped last against the view's size it would end at 99."""
    return dict(logits=np.array([[0.0, 3.0]], F32), regr=np.array([[0, 0, 0, 0, 0.0, 0.0, 10.0, 0.0]], F32), props=np.array([[60, 10, 90, 40]], F32),
                prop_cnt=1, image_hw=(50, 100), ratios_wh=(F32(2.0), F32(2.0)))
