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
    """-> boxes [N,nseg,seg_len,4], scores, labels, seg_cnt [N,nseg].  case["garbage"]: labels written round-robin into the slots past the counts (which
    already hold a box and a score that look valid)."""
    N = len(case["s"])
    parts = [_segments(case["b"][n], case["s"][n], case["l"][n], case["nseg"], case["seg_len"], counts=case.get("counts", [None] * N)[n]) for n in range(N)]
    B, S, Lb, cnt = (np.stack([p[i] for p in parts]) for i in range(4))
    if "garbage" in case:
        past = np.arange(case["seg_len"])[None, None, :] >= cnt[:, :, None]
        Lb[past] = np.resize(np.array(case["garbage"], np.int64), int(past.sum())).astype(np.int32)
    return B, S, Lb, cnt


def ref_post(case, nms_flags=0, det=100, cap=128, **kw):
    kw.setdefault("ncls", case.get("ncls", 81))
    return [rr.postprocess(case["b"][n], case["s"][n], case["l"][n], 0.4, det, cap, nms_flags, **kw) for n in range(len(case["s"]))]


# ===================================================================================================================== capacity and threshold edges
# Everything below is built on first use (lru_cache), never at import.  A = C = 1 rows: a level (1, n) is a row of exactly n logits and every label is 1.
KCAP = 1024                              # csrc/retinanet_ops.hip RETINA_KCAP: the largest top_n
TOP_NS = (1, 63, 64, 65, 1023, 1024)
BORDER_ROWS = (8191, 8192, 8193, 16383, 16384, 16385)
BORDER_TOP_N = 64
THRESHOLDS = (-1.0, 0.0, 1e-45, 1e-40, 1e-38, 1e-6, 0.3, 0.5, 0.7, 0.95, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0, 2.0)
SPECIALS = (-np.inf, -200.0, -104.0, -88.0, 0.0, 17.0, 100.0, np.inf, np.nan)


def candidates(row, thr=0.05):
    """How many logits of a row the reference's threshold test passes."""
    return int((ora.map_f32(np.asarray(row, F32).reshape(-1), 1) > F32(thr)).sum())


@functools.lru_cache(maxsize=None)
def topn_cases():
    """name -> (logits, A, C, top_n) on a single-slice row (4320 logits) and a four-slice row (25 200).  "topn_<k>": image 0 holds k + 37 distinct
    candidates, image 1 k // 2 distinct ones over a run of k - k // 2 + 30 equal ones, so that the cut falls inside the run.  "topn_1024_exact": 1024
    candidates in image 0, 1025 in image 1."""
    rng = np.random.default_rng(60)
    out = {}
    for k in TOP_NS:
        x = _rows(SHAPES[:2], 2, A, C)
        for lv in x:
            _scatter(lv[0].reshape(-1), rng, k + 37)
            f = lv[1].reshape(-1)
            d = k // 2
            pos = rng.choice(f.size, k + 30, replace=False)
            f[pos[:d]] = np.linspace(1.0, 4.0, d, dtype=F32)
            f[pos[d:]] = F32(0.5)
        out["topn_%d" % k] = (x, A, C, k)
    x = _rows(SHAPES[:2], 2, A, C)
    for lv in x:
        _scatter(lv[0].reshape(-1), rng, KCAP); _scatter(lv[1].reshape(-1), rng, KCAP + 1)
    out["topn_1024_exact"] = (x, A, C, KCAP)
    return out


def border_run(n):
    """The 100 indices centred on the first slice border, cut to the row."""
    return np.arange(SLICE - 50, min(SLICE + 50, n))


@functools.lru_cache(maxsize=None)
def border_cases():
    """name -> (logits, 1, 1, 64), rows of 8192 - 1 .. 2 * 8192 + 1 logits, N = 2; image 1 holds one candidate, on the row's last index.
    "border_distinct_<n>": distinct candidates on the last 20 indices of every slice and the first 20 of the next.
    "border_tie_<n>": a run of equal logits centred on index 8192 (and a second one on 16384) under so many distinct higher ones that the cut falls inside the
    first run: its lower indices win, across the border where the row has one."""
    rng = np.random.default_rng(61)
    out = {}
    for n in BORDER_ROWS:
        x = np.full((2, 1, n, 1), LOW, F32)
        idx = np.concatenate([np.arange(b - 20, b + 20) for b in range(SLICE, n + 20, SLICE)])
        idx = idx[idx < n]
        while True:
            v = rng.uniform(-2.5, 4.0, idx.size).astype(F32)
            if len(np.unique(ora.map_f32(v, 1))) == idx.size:
                break
        x[0, 0, idx, 0] = v
        x[1, 0, n - 1, 0] = 1.0
        out["border_distinct_%d" % n] = ([x], 1, 1, BORDER_TOP_N)
        x = np.full((2, 1, n, 1), LOW, F32)
        run = border_run(n)
        nd = 4 if run.size == 100 else BORDER_TOP_N - run.size + 1    # the cut falls inside the run: all but one of a short run, 60 of a whole one
        x[0, 0, 100:100 + nd, 0] = np.linspace(1.0, 3.0, nd, dtype=F32)
        x[0, 0, run, 0] = 0.5
        if n > 2 * SLICE - 50:
            x[0, 0, 2 * SLICE - 50:min(2 * SLICE + 50, n), 0] = 0.5   # the same score again around the second border: all of it loses
        x[1, 0, n - 1, 0] = 1.0
        out["border_tie_%d" % n] = ([x], 1, 1, BORDER_TOP_N)
    return out


GEOMETRY = ((5, 5000), (3, 3000), (7, 11), (2, 3), (1, 1))   # rows of 25 000, 9000, 77, 6 and 1 logits: 4, 2, 1, 1, 1 slices
GEOMETRY_TOP_N = 6
GEOMETRY_KINDS = (0, 1, GEOMETRY_TOP_N, GEOMETRY_TOP_N + 1, -1)   # candidates of a (level, image); -1: every logit


GEOMETRY_TABLE = ((4, 0, 3), (1, 4, 2), (2, 3, 4), (3, 1, 0), (0, 4, 1))   # [level][image] -> index into GEOMETRY_KINDS: both long rows pass whole once


def geometry_kind(l, n):
    return GEOMETRY_KINDS[GEOMETRY_TABLE[l][n]]


@functools.lru_cache(maxsize=None)
def geometry_case():
    """Five levels (the most the op takes), three images, A = C = 1; the candidate count of (level, image) is geometry_kind(l, n), cut to the row."""
    rng = np.random.default_rng(62)
    x = _rows(GEOMETRY, 3, 1, 1)
    for l, lv in enumerate(x):
        for n in range(3):
            f = lv[n].reshape(-1)
            k = geometry_kind(l, n)
            if k < 0:
                f[:] = rng.uniform(-2.0, 4.0, f.size).astype(F32)
            elif k:
                _scatter(f, rng, min(k, f.size))
    return x, 1, 1, GEOMETRY_TOP_N


def prefilter_of(thr):
    """The logit pre-filter of retina_select_launch as first built, in float32 like the launcher: logit(thr) - 0.25, None outside (0, 1)."""
    t = F32(thr)
    if not (t > 0 and t < 1):
        return None
    return F32(F32(np.log(t / (F32(1.0) - t))) - F32(0.25))


def _ord(x):
    u = int(np.array(x, F32).view(np.uint32))
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def _unord(o):
    u = (o & 0x7fffffff) if o & 0x80000000 else (~o & 0xffffffff)
    return np.array(u, np.uint32).view(F32)[()]


@functools.lru_cache(maxsize=None)
def crossing(thr):
    """(x_at, x_up): the consecutive floats with sigmoid(x_at) <= thr < sigmoid(x_up), by bisection over the floats of [-120, 120] (the sigmoid is monotone:
    threshold_logits() checks it around its own crossing, threshold_case() around this one).  None when every float passes or none does."""
    def passes(x):
        return bool(ora.map_f32(np.array([x], F32), 1)[0] > F32(thr))
    lo, hi = _ord(F32(-120.0)), _ord(F32(120.0))
    if passes(_unord(lo)) or not passes(_unord(hi)):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if passes(_unord(mid)):
            hi = mid
        else:
            lo = mid
    return _unord(lo), _unord(hi)


def _threshold_filler(thr):
    """LOW where the threshold drops it, NaN (which no threshold passes) under the smaller thresholds: the row then holds fewer than 1024 numbers and the
    selected list is the whole set that passed."""
    return LOW if ora.map_f32(np.array([LOW], F32), 1)[0] <= F32(thr) else F32(np.nan)


@functools.lru_cache(maxsize=None)
def threshold_case(thr):
    """-> (logits, 1, 1, 1024): one row of 4000 with 16 consecutive floats around the crossing of thr, 512 logits over [pre-filter - 1, pre-filter + 1]
    and SPECIALS, shuffled."""
    rng = np.random.default_rng(63)
    vals = [np.array(SPECIALS, F32)]
    c = crossing(thr)
    if c is not None:
        w = np.array([_next(c[0], -k) for k in range(7, 0, -1)] + [c[0], c[1]] + [_next(c[1], k) for k in range(1, 8)], F32)
        p = ora.map_f32(w, 1)
        assert (np.diff(p) >= 0).all() and (p[:8] <= F32(thr)).all() and (p[8:] > F32(thr)).all()
        vals.append(w)
    pre = prefilter_of(thr)
    if pre is not None:
        vals.append((np.float64(pre) + np.linspace(-1.0, 1.0, 512)).astype(F32))
    vals = np.concatenate(vals)
    row = np.full(4000, _threshold_filler(thr), F32)
    row[rng.choice(row.size, vals.size, replace=False)] = vals
    return [row.reshape(1, 1, 4000, 1)], 1, 1, KCAP


TOWER = tuple(a * C for a in range(A))   # the channel of class 1 of each of the nine anchors of a cell


@functools.lru_cache(maxsize=None)
def decode_edge_case(kind):
    """-> (logits, deltas, anchors, image_hw) of decode_case() with every anchor of cell (0, 0) selected (class 1) on each level.
    "tiny_image": a 1 x 1 image.  "zero_deltas": all deltas 0, the decoded box is the clipped anchor.  "special_deltas": NaN and +-inf in dx, dy, dw of
    those nine anchors."""
    logits, deltas, anchors, hw = decode_case()
    logits = [lg.copy() for lg in logits]
    for lg in logits:
        lg[:, 0, 0, list(TOWER)] = np.linspace(3.0, 4.0, A, dtype=F32)
    if kind == "tiny_image":
        hw = np.array([[1, 1], [1, 1]], np.int32)
    elif kind == "zero_deltas":
        deltas = [np.zeros_like(d) for d in deltas]
    elif kind == "special_deltas":
        deltas = [d.copy() for d in deltas]
        nan, inf = F32(np.nan), F32(np.inf)
        for d in deltas:   # (anchor, component, value): dx, dy, dw, dh are components 0..3
            for a, k, v in ((1, 0, nan), (2, 2, nan), (3, 0, inf), (4, 0, -inf), (5, 2, inf), (6, 2, -inf), (7, 1, nan), (8, 1, inf)):
                d[:, 0, 0, a * 4 + k] = v
    else:
        raise KeyError(kind)
    return logits, deltas, anchors, hw


@functools.lru_cache(maxsize=None)
def min_size_edge():
    """(m, m_up): the smaller side (+1) of the best box of level 0, image 0 of the zero-delta case and the next float: min_size m keeps that box, m_up drops it."""
    logits, deltas, anchors, hw = decode_edge_case("zero_deltas")
    s, i = rr.select_level(logits[0][0])
    b, _, _ = rr.decode_level(s[:1], i[:1], deltas[0][0], anchors[0], hw[0][1], hw[0][0])
    m = min(b[0, 2] - b[0, 0] + F32(1), b[0, 3] - b[0, 1] + F32(1))
    return F32(m), _next(m)


# --------------------------------------------------------------------------------------------------------------------- retina_postprocess
FULL = 8192                              # csrc/retinanet_ops.hip RETINA_MAX_SLOTS
FULL_SEG = dict(nseg=8, seg_len=1024)


@functools.lru_cache(maxsize=None)
def full_cases():
    """Every one of the 8192 slots valid.  "full_one_class"; "full_100_then_8092": class 2 starts inside word 1 and spans 127 words;
    "full_255_classes": ncls 256 with 4055 of class 1, 37 of class 254, 4100 of class 255 (which starts inside word 63 and spans 65 words);
    "batch_8192_0_1": three images holding 8192, 0 and 1 candidates."""
    rng = np.random.default_rng(64)
    b = _clustered(rng, FULL, centres=40, spread=25.0); s = rng.uniform(0.05, 1.0, FULL).astype(F32)
    out = {}
    out["full_one_class"] = dict(b=[b], s=[s], l=[np.full(FULL, 17, np.int32)], **FULL_SEG)
    out["full_100_then_8092"] = dict(b=[b], s=[s], l=[np.r_[np.full(100, 1), np.full(8092, 2)].astype(np.int32)], **FULL_SEG)
    out["full_255_classes"] = dict(b=[b], s=[s], l=[np.r_[np.full(37, 254), np.full(4100, 255), np.full(4055, 1)].astype(np.int32)], ncls=256, **FULL_SEG)
    out["batch_8192_0_1"] = dict(b=[b, b[:0], b[5:6]], s=[s, s[:0], s[5:6]], l=[np.full(FULL, 17, np.int32), np.zeros(0, np.int32), np.full(1, 80, np.int32)],
                                 counts=[None, [0] * 8, [0, 0, 0, 1, 0, 0, 0, 0]], **FULL_SEG)
    for c in out.values():
        for a in c["b"] + c["s"] + c["l"]:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _full_image_ref(name, n, det, cap):
    c = full_cases()[name]
    return rr.postprocess(c["b"][n], c["s"][n], c["l"][n], 0.4, det, cap, 0, ncls=c.get("ncls", 81))


def full_ref(name, det, cap):
    """The reference of a full case, computed once per (image, det, cap): image 0 of the batch case is full_one_class's."""
    c = full_cases()[name]
    return [_full_image_ref("full_one_class" if name == "batch_8192_0_1" and n == 0 else name, n, det, cap) for n in range(len(c["s"]))]


def class_reach(case, cls, n=0, thr=0.4):
    """What the greedy scan of one class has to carry, from the oracle's NMS and plain float32 IoUs: dict(s, e: the class's range in the engine's sorted order
    (class asc, score desc, slot asc); words; far: a kept box among the first 64 of the class overlaps (IoU > thr) one more than 4096 ranks later;
    upper: ... one in a word 64 or more after the class's first; last: ... one in the class's last word)."""
    b, s, lab = case["b"][n], case["s"][n], case["l"][n]
    nc = case.get("ncls", 81) - 1
    valid = (lab >= 1) & (lab <= nc)
    start = int((valid & (lab < cls)).sum())
    idx = np.flatnonzero(lab == cls)
    idx = idx[np.lexsort((idx, -s[idx].astype(np.float64)))]
    srt = np.sort(idx)                   # ora.nms breaks score ties by position: hand it the class in slot order
    kept = set(srt[ora.nms(b[srt], s[srt], thr, 1, 0)].tolist())
    e = start + idx.size
    w0 = start >> 6
    word = (start + np.arange(idx.size)) >> 6
    bb = b[idx]
    area = (bb[:, 2] - bb[:, 0] + F32(1)) * (bb[:, 3] - bb[:, 1] + F32(1))
    far = upper = last = False
    for r in range(min(64, idx.size)):
        if int(idx[r]) not in kept:
            continue
        w = np.clip(np.minimum(bb[r, 2], bb[:, 2]) - np.maximum(bb[r, 0], bb[:, 0]) + F32(1), 0, None)
        h = np.clip(np.minimum(bb[r, 3], bb[:, 3]) - np.maximum(bb[r, 1], bb[:, 1]) + F32(1), 0, None)
        inter = w * h
        hit = inter / (area[r] + area - inter) > F32(thr)
        hit[:r + 1] = False
        far |= bool(hit[r + 4097:].any())
        upper |= bool(hit[word - w0 >= 64].any())
        last |= bool(hit[word == word[-1]].any())
    return dict(s=start, e=e, words=int(word[-1] - w0 + 1), far=far, upper=upper, last=last)


GRID = np.array([[x * 30, y * 30, x * 30 + 20, y * 30 + 20] for y in range(15) for x in range(15)], F32)   # 225 disjoint boxes: NMS keeps every one
CUT_K = 40


@functools.lru_cache(maxsize=None)
def edge_post_cases():
    """name -> case dict (as post_cases()).
    "ncls_2": one class.  "labels_out_of_range": labels 0, -1, ncls and 300 inside the valid counts, each on the box of an in-range candidate of a lower score
    that it would suppress if it were counted into that class; the slots past the counts hold garbage of labels in and out of range.
    "cut_k40" / "cut_k40_zeros": 40 disjoint boxes, all kept; the 39th and 40th scores tie ("zeros": the scores 31..34 are +-0.0, the rest under them
    negative), all tied boxes in one class."""
    rng = np.random.default_rng(65)
    out = {}
    b = _clustered(rng, 60, centres=4, spread=8.0, extent=300.0); s = rng.uniform(0.05, 1.0, 60).astype(F32)
    out["ncls_2"] = dict(b=[b], s=[s], l=[np.ones(60, np.int32)], nseg=3, seg_len=25, counts=[[25, 10, 25]], ncls=2, garbage=(1, 0, 2, -1))
    for ncls in (2, 81):
        bb = np.repeat(GRID[:6], 2, 0)                                   # pairs of identical boxes
        ss = np.tile(np.array([0.9, 0.6], F32), 6) - np.repeat(np.arange(6), 2).astype(F32) * F32(0.01)
        ll = np.tile(np.array([0, 1], np.int32), 6)                      # the better of each pair carries the bad label, the other label 1
        ll[0::2] = [0, -1, ncls, 300, -2 ** 31, 2 ** 31 - 1]
        out["labels_out_of_range_ncls_%d" % ncls] = dict(b=[bb], s=[ss], l=[ll], nseg=2, seg_len=8, counts=[[7, 5]], ncls=ncls, garbage=(1, 0, ncls, -1, 300, ncls - 1))
    perm = rng.permutation(CUT_K)
    sc = np.concatenate([np.linspace(0.99, 0.2, CUT_K - 2), np.full(2, 0.1)]).astype(F32)
    lab = rng.integers(1, 81, CUT_K).astype(np.int32); lab[-2:] = 7
    out["cut_k40"] = dict(b=[GRID[:CUT_K][perm]], s=[sc[perm]], l=[lab[perm]], nseg=4, seg_len=12, counts=[[12, 4, 12, 12]])
    sc = np.concatenate([np.linspace(0.99, 0.2, 30), [0.0, -0.0, -0.0, 0.0], np.linspace(-0.1, -0.4, 4), [-0.5, -0.5]]).astype(F32)
    lab = rng.integers(1, 81, CUT_K).astype(np.int32); lab[30:] = 7
    out["cut_k40_zeros"] = dict(b=[GRID[:CUT_K][perm]], s=[sc[perm]], l=[lab[perm]], nseg=4, seg_len=12, counts=[[12, 4, 12, 12]])
    return out
