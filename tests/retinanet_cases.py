"""Crafted inputs of the RetinaNet tail ops, shared by tests/test_retinanet_ops_gpu.py (kernels against the reference) and tests/test_retinanet_cpu.py
(the reference alone: every case discriminates the rule it is named for)."""
import functools

import numpy as np

import retinanet_ref as rr
from oracle import ora

F32 = np.float32
A, C = 9, 80
SHAPES = ((5, 7), (3, 2), (1, 1))       # level maps of the select cases, N = 2, top_n 1000: rows of 25 200 (four slices of 8192), 4320 and 720 logits
TOP_N = 1000
TOY = ((4, 3),)                         # A = 2, C = 3, top_n 8: 72 logits
LONG = ((40, 41),)                      # 1 180 800 logits: 145 slices of 8192, the last one short (1152 logits)
SLICE = 8192                            # the kernel's slice length (csrc/retinanet_ops.hip RETINA_SLICE): a row longer than this takes the multi-slice path
LOW = F32(-10.0)                        # under any pre-filter: sigmoid 4.5e-5


def _next(x, k=1):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return x


@functools.lru_cache(maxsize=None)
def threshold_logits(thr=0.05):
    """(x_at, x_up): consecutive floats with sigmoid(x_at) <= thr < sigmoid(x_up); exact is True when sigmoid(x_at) == float32(thr)."""
    x0 = F32(np.log(thr / (1.0 - thr)))
    xs = [x0]
    for _ in range(600):
        xs.append(_next(xs[-1]))
    xs = np.array(sorted(set([_next(x0, -k) for k in range(1, 600)] + xs)), F32)
    p = ora.map_f32(xs, 1)
    assert (np.diff(p) >= 0).all()
    i = int(np.flatnonzero(p > F32(thr))[0])
    assert i > 0
    return xs[i - 1], xs[i], bool(p[i - 1] == F32(thr))


@functools.lru_cache(maxsize=None)
def same_sigmoid_logits():
    """Two different logits with one sigmoid."""
    xs = np.array([_next(F32(2.0), k) for k in range(64)], F32)
    p = ora.map_f32(xs, 1)
    for i in range(len(xs) - 1):
        if p[i] == p[i + 1]:
            return xs[i], xs[i + 1]
    raise AssertionError("no pair of neighbours shares a sigmoid")


def _rows(shapes, N, a, c, fill=LOW):
    return [np.full((N, h, w, a * c), fill, F32) for h, w in shapes]


def _scatter(arr, rng, count, lo=-2.5, hi=4.0):
    """`count` distinct random logits (distinct sigmoids) at random places of one row (arr: a flat view)."""
    pos = rng.choice(arr.size, count, replace=False)
    while True:
        v = rng.uniform(lo, hi, count).astype(F32)
        if len(np.unique(ora.map_f32(v, 1))) == count:
            break
    arr[pos] = v
    return pos


def select_cases():
    """name -> (logits per level, A, C, top_n)."""
    rng = np.random.default_rng(20)
    out = {}
    out["none"] = (_rows(SHAPES, 2, A, C), A, C, TOP_N)
    x = _rows(SHAPES, 2, A, C, F32(-3.0))          # past the logit pre-filter, under the threshold: sigmoid 0.0474
    out["none_past_prefilter"] = (x, A, C, TOP_N)
    x = _rows(SHAPES, 2, A, C)
    _scatter(x[0][0].reshape(-1), rng, TOP_N); _scatter(x[0][1].reshape(-1), rng, TOP_N + 1)
    _scatter(x[1][0].reshape(-1), rng, TOP_N + 1); _scatter(x[1][1].reshape(-1), rng, TOP_N)
    _scatter(x[2][0].reshape(-1), rng, 720); _scatter(x[2][1].reshape(-1), rng, 1)
    out["exactly_top_n_and_one_more"] = (x, A, C, TOP_N)
    out["every_logit_passes"] = ([rng.uniform(-2.0, 4.0, (2, h, w, A * C)).astype(F32) for h, w in SHAPES], A, C, TOP_N)
    x_at, x_up, _ = threshold_logits()
    x = _rows(SHAPES, 2, A, C)
    for lv in x:
        for n in range(2):
            f = lv[n].reshape(-1)
            pos = rng.choice(f.size, 40, replace=False)
            f[pos[:20]] = x_at; f[pos[20:]] = x_up
    out["threshold_edge"] = (x, A, C, TOP_N)
    x = _rows(SHAPES, 2, A, C)
    for n in range(2):   # 900 distinct high logits, then a run of 300 equal ones across the cut (and across the slices)
        f = x[0][n].reshape(-1)
        pos = rng.choice(f.size, 1200, replace=False)
        f[pos[:900]] = np.linspace(1.0, 4.0, 900, dtype=F32)
        f[pos[900:]] = F32(0.5)
        g = x[1][n].reshape(-1)   # the whole level equal: the first top_n flat indices win
        g[:] = F32(0.25)
    out["equal_run_at_cut"] = (x, A, C, TOP_N)
    xa, xb = same_sigmoid_logits()
    x = _rows(SHAPES, 2, A, C)
    for lv in x:
        for n in range(2):
            f = lv[n].reshape(-1)
            pos = np.sort(rng.choice(f.size, 6, replace=False))
            f[pos] = [xb, xa, xb, xa, xa, xb]   # the larger LOGIT first: ranking logits instead of sigmoids would reorder them
    out["same_sigmoid"] = (x, A, C, TOP_N)
    x = _rows(SHAPES, 2, A, C)
    for lv in x:
        for n in range(2):
            f = lv[n].reshape(-1)
            f[rng.choice(f.size, 30, replace=False)] = F32(-np.inf)
            f[rng.choice(f.size, 30, replace=False)] = F32(np.inf)
            f[rng.choice(f.size, 30, replace=False)] = F32(1.0)
    out["inf_logits"] = (x, A, C, TOP_N)
    # toy: 72 logits, top_n 8
    t = rng.uniform(-4.0, 1.0, (2, 4, 3, 6)).astype(F32)
    out["toy"] = ([t], 2, 3, 8)
    t = np.full((2, 4, 3, 6), LOW, F32); t[0, 1, 1, 3] = 0.0; t[1] = 0.0
    out["toy_one_and_all_equal"] = ([t], 2, 3, 8)
    return out


def long_cases():
    rng = np.random.default_rng(21)
    out = {}
    x = _rows(LONG, 1, A, C)
    f = x[0][0].reshape(-1)
    last = (f.size - 1) // SLICE * SLICE
    _scatter(f[last:], rng, 1100)
    out["long_all_in_last_slice"] = (x, A, C, TOP_N)
    x = _rows(LONG, 1, A, C)
    f = x[0][0].reshape(-1)
    f[(np.arange(3000) * (f.size // 3000) + 17)] = np.tile(np.linspace(-1.0, 3.0, 1500, dtype=F32), 2)   # every value twice: ties across slices
    out["long_spread"] = (x, A, C, TOP_N)
    return out


def decode_case():
    """logits, deltas, anchors per level, image_hw: anchors outside the image and deltas at the log(1000/16) clamp among the selected."""
    rng = np.random.default_rng(22)
    logits = [rng.uniform(-6.0, 0.0, (2, h, w, A * C)).astype(F32) for h, w in SHAPES]
    deltas = [(rng.standard_normal((2, h, w, A * 4)) * 3.0).astype(F32) for h, w in SHAPES]
    for d in deltas:
        d[:, 0, 0, 2] = 5.0 * 4.2; d[:, 0, 0, 3] = 5.0 * 4.135166556742356   # anchor 0 of cell (0, 0): over and on the clamp
    for lg in logits:
        lg[:, 0, 0, :3] = 3.0   # ... and selected
    anchors = [rr.level_anchors(l, h, w) for l, (h, w) in enumerate(SHAPES)]
    hw = np.array([[37, 50], [40, 56]], np.int32)
    return logits, deltas, anchors, hw


def _clustered(rng, n, centres=12, spread=6.0, size=(20.0, 60.0), extent=600.0):
    c = rng.uniform(50, extent - 50, (centres, 2))
    k = rng.integers(0, centres, n)
    ctr = c[k] + rng.normal(0, spread, (n, 2))
    wh = rng.uniform(size[0], size[1], (n, 2))
    b = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    return np.round(np.clip(b, 0, extent - 1)).astype(F32)


def _segments(boxes, scores, labels, nseg, seg_len, rng=None, counts=None):
    """Pack one image's candidates into nseg lists of seg_len slots: list s takes counts[s] (default: filled front to back); slots past a count hold garbage."""
    n = len(scores)
    if counts is None:
        counts = [min(seg_len, max(0, n - s * seg_len)) for s in range(nseg)]
    assert sum(counts) == n and max(counts) <= seg_len
    B = np.full((nseg, seg_len, 4), 7.0, F32); S = np.full((nseg, seg_len), 0.99, F32); Lb = np.full((nseg, seg_len), 1, np.int32)
    o = 0
    for s, c in enumerate(counts):
        B[s, :c] = boxes[o:o + c]; S[s, :c] = scores[o:o + c]; Lb[s, :c] = labels[o:o + c]
        o += c
    return B, S, Lb, np.array(counts, np.int32)


def iou_04_pair():
    """IoU exactly float32(0.4) with the legacy +1: 7 x 5 boxes three columns apart, 20 / 50."""
    return np.array([[0, 0, 6, 4], [3, 0, 9, 4]], F32)


def post_cases():
    """name -> dict(boxes, scores, labels per image (lists), nseg, seg_len, counts (optional), det, cap): kwargs of run_post / ref_post."""
    rng = np.random.default_rng(23)
    out = {}
    b = _clustered(rng, 5000, centres=40, spread=25.0); s = rng.uniform(0.05, 1.0, 5000).astype(F32)
    out["one_class_5000"] = dict(b=[b], s=[s], l=[np.full(5000, 17, np.int32)], nseg=5, seg_len=1000)
    s2 = (np.round(s * 64) / 64).astype(F32)   # heavy score ties: the slot decides
    out["eighty_classes_5000"] = dict(b=[b, b[::-1].copy()], s=[s2, s], l=[rng.integers(1, 81, 5000).astype(np.int32), (np.arange(5000) % 80 + 1).astype(np.int32)],
                                      nseg=5, seg_len=1000)
    bb = np.array([[10, 10, 50, 50], [10, 10, 50, 50], [10, 10, 50, 50]], F32)
    out["identical_boxes_two_classes"] = dict(b=[bb], s=[np.array([0.9, 0.8, 0.7], F32)], l=[np.array([3, 5, 3], np.int32)], nseg=2, seg_len=4, counts=[[2, 1]])
    p = iou_04_pair()
    out["iou_exactly_thr"] = dict(b=[np.concatenate([p, p + 100])], s=[np.array([0.9, 0.8, 0.6, 0.7], F32)], l=[np.array([2, 2, 9, 9], np.int32)], nseg=1, seg_len=4)
    # more than 100 kept, a tie group across the 100th score: disjoint boxes, nothing suppressed
    g = np.array([[x * 30, y * 30, x * 30 + 20, y * 30 + 20] for y in range(15) for x in range(15)], F32)
    sc = np.concatenate([np.linspace(0.99, 0.6, 95), np.full(20, 0.5), np.linspace(0.4, 0.1, 110)]).astype(F32)
    perm = rng.permutation(225)
    out["cut_tie_group_fits_cap"] = dict(b=[g[perm]], s=[sc[perm]], l=[rng.integers(1, 81, 225).astype(np.int32)], nseg=5, seg_len=50, counts=[[45, 50, 30, 50, 50]])
    sc = np.concatenate([np.linspace(0.99, 0.6, 95), np.full(60, 0.5), np.linspace(0.4, 0.1, 70)]).astype(F32)
    out["cut_tie_group_over_cap"] = dict(b=[g[perm]], s=[sc[perm]], l=[rng.integers(1, 81, 225).astype(np.int32)], nseg=5, seg_len=50, counts=[[45, 50, 30, 50, 50]])
    out["fewer_than_det"] = dict(b=[g[:40], g[:0]], s=[sc[:40], sc[:0]], l=[rng.integers(1, 81, 40).astype(np.int32), np.zeros(0, np.int32)], nseg=3, seg_len=20,
                                 counts=[[20, 0, 20], [0, 0, 0]])
    out["zero_candidates"] = dict(b=[g[:0]], s=[sc[:0]], l=[np.zeros(0, np.int32)], nseg=5, seg_len=1000)
    return out


def pack_post(case, rng=None):
    """-> boxes [N,nseg,seg_len,4], scores, labels, seg_cnt [N,nseg]"""
    N = len(case["s"])
    parts = [_segments(case["b"][n], case["s"][n], case["l"][n], case["nseg"], case["seg_len"], counts=case.get("counts", [None] * N)[n]) for n in range(N)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


def ref_post(case, nms_flags=0, det=100, cap=128, **kw):
    return [rr.postprocess(case["b"][n], case["s"][n], case["l"][n], 0.4, det, cap, nms_flags, **kw) for n in range(len(case["s"]))]
