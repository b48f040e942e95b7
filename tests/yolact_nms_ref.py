"""Restatement of the two Yolact suppression rules the default path does not run ([UPSTREAM-RECALL] dbolya/yolact layers/functions/detection.py:
Detect.cc_fast_nms and Detect.traditional_nms with utils/cython_nms.pyx), in numpy fp32, one IEEE operation per upstream operation, plus the
crafted decision cases shared by the CPU and GPU tests.  Softmax and box decode come from the oracle (ora.softmax / ora.yolact_decode), as for
the default rule (ora.yolact_detect).  DESIGN.md 20 states the contract; the fork notes are repeated where they bite.

Every function takes ONE image: prob [P, ncls] (softmax probabilities, column 0 = background), boxes [P, 4] (decoded relative xyxy),
mask [P, md]; and returns (dict(box, score, cls, mask, prior), nms_total[, overflow]) with cls 0-based over the foreground classes.
"""
import numpy as np

F = np.float32


def _order(score, prior):
    """(score descending, prior index ascending): the project's key contract (upstream's sort / argsort leave ties unspecified)"""
    return np.lexsort((prior, -score))


def jaccard(b):
    """box_utils.jaccard of a box list with itself, fp32: plain areas (no +1), IEEE division; entry [i, j] = IoU(box i, box j)"""
    b = np.asarray(b, F)
    mx2 = np.minimum(b[:, None, 2], b[None, :, 2]); mx1 = np.maximum(b[:, None, 0], b[None, :, 0])
    my2 = np.minimum(b[:, None, 3], b[None, :, 3]); my1 = np.maximum(b[:, None, 1], b[None, :, 1])
    iw = mx2 - mx1; ih = my2 - my1
    iw = np.where(iw > 0, iw, F(0)); ih = np.where(ih > 0, ih, F(0))
    inter = iw * ih
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    uni = area[:, None] + area[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / uni).astype(F)


def _rows(idx, score, cls, boxes, mask):
    idx = np.asarray(idx, np.int64)
    return dict(box=boxes[idx].astype(F), score=np.asarray(score, F), cls=np.asarray(cls, np.int32), mask=mask[idx].astype(F),
                prior=idx.astype(np.int32))


def cc_fast_nms(prob, boxes, mask, conf_thresh=0.05, nms_thr=0.5, top_k=200, max_det=100):
    prob = np.asarray(prob, F); boxes = np.asarray(boxes, F); mask = np.asarray(mask, F)
    fg = prob[:, 1:]
    keep = np.nonzero(fg.max(1) > F(conf_thresh))[0]          # Detect.detect's pre-filter
    if keep.size == 0:
        return _rows([], [], [], boxes, mask), 0
    score = fg[keep].max(1)
    cls = fg[keep].argmax(1)                                   # fork note: torch.max's tie index is unspecified; here the LOWEST class
    o = _order(score, keep)[:top_k]
    idx, score, cls = keep[o], score[o], cls[o]
    iou = np.triu(jaccard(boxes[idx]), 1)
    ok = np.ones(len(idx), bool)
    for j in range(1, len(idx)):                               # iou.max(dim=0) <= thr; a NaN in the column drops the box
        col = iou[:j, j]
        ok[j] = not np.isnan(col).any() and col.max() <= F(nms_thr)
    idx, score, cls = idx[ok], score[ok], cls[ok]
    total = len(idx)
    # deliberate deviation: upstream returns every survivor (<= top_k); the engine's rows hold the best max_det
    return _rows(idx[:max_det], score[:max_det], cls[:max_det], boxes, mask), total


def cnms_keep(b, thr):
    """utils/cython_nms.pyx over boxes already in visiting order: +1 areas, w = max(0, xx2 - xx1 + 1), ovr = inter / (area_i + area_j - inter),
    a later box goes iff ovr >= thr.  Returns the kept positions."""
    b = np.asarray(b, F)
    n = len(b)
    one = F(1)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    gone = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if gone[i]:
            continue
        kept.append(i)
        r = slice(i + 1, n)
        w = np.minimum(b[i, 2], b[r, 2]) - np.maximum(b[i, 0], b[r, 0]) + one
        h = np.minimum(b[i, 3], b[r, 3]) - np.maximum(b[i, 1], b[r, 1]) + one
        w = np.where(w > 0, w, F(0)); h = np.where(h > 0, h, F(0))
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (area[i] + area[r] - inter)
        gone[r] |= ovr >= F(thr)
    return np.asarray(kept, np.int64)


def traditional_nms(prob, boxes, mask, conf_thresh=0.05, nms_thr=0.5, max_det=100, max_size=550, cap=None):
    """cap=None: upstream (every candidate of a class is visited).  cap=k: the engine's form -- the k best candidates of a class are visited -- and
    the third result is the cap lemma's flag: some class held MORE than k candidates and FEWER than max_det of its first k survived.  With the flag
    clear the result equals cap=None's: a class within the cap is not truncated, and behind max_det survivors of one class every unvisited candidate
    of it scores lower than those max_det detections, so it cannot enter the final cut."""
    prob = np.asarray(prob, F); boxes = np.asarray(boxes, F); mask = np.asarray(mask, F)
    scaled = boxes * F(max_size)                               # upstream multiplies before cnms
    idx_all, score_all, cls_all, rank_all = [], [], [], []
    overflow = 0
    for c in range(prob.shape[1] - 1):
        s = prob[:, c + 1]
        cand = np.nonzero(s > F(conf_thresh))[0]               # implies the pre-filter: such a prior's best class is above the threshold too
        if cand.size == 0:
            continue
        cand = cand[_order(s[cand], cand)]                     # fork note: argsort()[::-1] leaves ties unspecified; the key contract applies
        ncand = len(cand)
        if cap is not None:
            cand = cand[:cap]
        kept = cnms_keep(scaled[cand], nms_thr)
        if cap is not None and ncand > cap and len(kept) < max_det:
            overflow = 1
        idx_all.append(cand[kept]); score_all.append(s[cand[kept]]); cls_all.append(np.full(len(kept), c)); rank_all.append(np.arange(len(kept)))
    if not idx_all:
        return _rows([], [], [], boxes, mask), 0, overflow
    idx = np.concatenate(idx_all); score = np.concatenate(score_all); cls = np.concatenate(cls_all); rank = np.concatenate(rank_all)
    o = np.lexsort((rank, cls, -score))[:max_det]              # (score desc, class asc, rank in class asc)
    return _rows(idx[o], score[o], cls[o], boxes, mask), len(idx), overflow


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("prior", "cls", "score", "box", "mask"))


# ------------------------------------------------------------------------------------------------ crafted cases
# Boxes are given in "pixels" of a 512-wide canvas (max_size = 512) on dyadic coordinates, as PRIORS with zero regressions: decode reproduces them
# exactly (cx - w / 2 and w + x1 are exact on dyadic values), and both IoU arithmetics are exact on them.
CASE_MAX_SIZE = 512


def _case(boxes_px, hot, ncls=6, md=4, **params):
    """boxes_px [P][4] xyxy in pixels; hot: per prior a dict {class (1-based): logit}; background logit 0, every other class -12."""
    b = np.asarray(boxes_px, np.float64) / CASE_MAX_SIZE
    P = len(b)
    priors = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(F)
    conf = np.full((1, P, ncls), -12.0, F)
    conf[..., 0] = 0.0
    for p, h in enumerate(hot):
        for c, v in h.items():
            conf[0, p, c] = v
    loc = np.zeros((1, P, 4), F)
    mask = np.tanh(np.arange(P * md, dtype=F).reshape(1, P, md) * F(0.37) - F(1)).astype(F)
    par = dict(conf_thresh=0.05, nms_thr=0.5, top_k=200, max_det=100, max_size=CASE_MAX_SIZE)
    par.update(params)
    return dict(conf=conf, loc=loc, mask=mask, priors=priors, params=par)


def _o(box, dx=64, dy=64):
    return [box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy]


def case_chain():
    """A suppresses B, B overlaps C, A does not overlap C: greedy keeps C, fast NMS drops it"""
    return _case([_o([0, 0, 10, 10]), _o([3, 0, 13, 10]), _o([6, 0, 16, 10])], [{2: 5.0}, {2: 4.0}, {2: 3.0}])


def case_two_classes():
    """one box twice, in two classes: per-class rules keep both, the cross-class rule keeps one"""
    return _case([_o([0, 0, 16, 16]), _o([0, 0, 16, 16])], [{1: 5.0}, {3: 4.0}])


def case_edge_plus_one():
    """+1 on the scaled boxes: areas 16 and 8, intersection 8, ovr = 0.5 exactly: >= suppresses, > would not (plain IoU: 3/9)"""
    return _case([_o([0, 0, 3, 3]), _o([0, 0, 3, 1])], [{2: 5.0}, {2: 4.0}])


def case_edge_plain():
    """the same pair with nms_thr = fl(3 / 9), its plain IoU: mode 1's <= keeps the second box, < would drop it"""
    c = case_edge_plus_one()
    c["params"]["nms_thr"] = float(F(3.0) / F(9.0))
    return c


def case_arithmetic():
    """plain IoU 2/4 = 0.5 (kept by <=), +1 on the scaled boxes 6/9 (suppressed): the two arithmetics disagree"""
    return _case([_o([0, 0, 2, 2]), _o([0, 0, 2, 1])], [{2: 5.0}, {2: 4.0}])


def case_class_tie():
    """a prior whose best score is attained by classes 2 and 4 (0-based 1 and 3): the cross-class rule labels it with the lower"""
    return _case([_o([0, 0, 16, 16]), _o([100, 0, 116, 16])], [{2: 5.0, 4: 5.0}, {3: -1.0}])


def case_at_threshold(softmax):
    """prior 0 passes the pre-filter on class 2; its class-4 score IS conf_thresh, so class 4 has no candidate under the traditional rule (the test
    is >), while the default rule ranks the prior in every class"""
    c = _case([_o([0, 0, 16, 16]), _o([100, 0, 116, 16])], [{2: 3.0, 4: 1.0}, {3: 4.0}])
    c["params"]["conf_thresh"] = float(softmax(c["conf"][0])[0, 4])
    return c


def case_cut(n=30, max_det=20):
    """n disjoint boxes of one class and distinct scores, max_det < n: the cut and nms_total"""
    boxes = [_o([20 * (i % 8), 20 * (i // 8), 20 * (i % 8) + 10, 20 * (i // 8) + 10]) for i in range(n)]
    return _case(boxes, [{1 + i % 3: 6.0 - 0.05 * i} for i in range(n)], max_det=max_det)


def case_cap_hidden(cap=64):
    """the cap lemma's bad case: `cap` identical boxes, then a disjoint one behind them: the truncated result lacks it and the flag is set"""
    boxes = [_o([0, 0, 16, 16])] * cap + [_o([200, 200, 216, 216])]
    return _case(boxes, [{2: 6.0 - 0.01 * i} for i in range(cap + 1)])


def case_cap_harmless(cap=64, max_det=32):
    """cap + 1 disjoint boxes with max_det <= cap: more candidates than the cap, yet max_det of the visited ones survive: flag clear, same result"""
    n = cap + 1
    boxes = [_o([24 * (i % 16), 24 * (i // 16), 24 * (i % 16) + 10, 24 * (i // 16) + 10], 8, 8) for i in range(n)]
    return _case(boxes, [{2: 6.0 - 0.01 * i} for i in range(n)], max_det=max_det)


def case_one_class_count(m, extra=0, ncls=4):
    """m candidates in class 1 on a jittered grid of overlapping boxes (distinct scores), `extra` more in class 2"""
    rng = np.random.default_rng(1000 + m)
    n = m + extra
    x = rng.integers(0, 120, n); y = rng.integers(0, 120, n); w = rng.integers(8, 60, n); h = rng.integers(8, 60, n)
    boxes = np.stack([x, y, x + w, y + h], 1).tolist()
    lg = 7.0 - 6.0 * np.arange(n) / max(n, 1)
    hot = [{1: float(lg[i])} if i < m else {2: float(lg[i])} for i in range(n)]
    return _case(boxes, hot, ncls=ncls)


def random_inputs(rng, N, P, ncls=81, md=32, hot=0.25):
    """clustered random heads: a `hot` fraction of the priors carries one boosted class, a few classes collect most of them"""
    conf = rng.standard_normal((N, P, ncls)).astype(F)
    conf[..., 0] += 4.0
    hotm = rng.uniform(0, 1, (N, P)) < hot
    cls = 1 + np.minimum(rng.integers(0, ncls - 1, (N, P)), rng.integers(0, ncls - 1, (N, P)))
    boost = rng.uniform(3, 9, (N, P)).astype(F)
    for n in range(N):
        idx = np.nonzero(hotm[n])[0]
        conf[n, idx, cls[n, idx]] += boost[n, idx]
    ctr = rng.uniform(0.2, 0.8, (P, 2))
    ctr[1::3] = ctr[(np.arange(P)[1::3] - 1)] + rng.uniform(-0.02, 0.02, (len(ctr[1::3]), 2))
    priors = np.concatenate([ctr, rng.uniform(0.05, 0.3, (P, 2))], 1).astype(F)
    loc = (rng.standard_normal((N, P, 4)) * 0.3).astype(F)
    mask = np.tanh(rng.standard_normal((N, P, md))).astype(F)
    return conf, loc, mask, priors


def run_ref(mode, prob, boxes, mask, conf_thresh=0.05, nms_thr=0.5, top_k=200, max_det=100, max_size=550, cap=None):
    """-> (detections, nms_total, overflow) of one image in nms_mode 1 or 2"""
    if mode == 1:
        d, t = cc_fast_nms(prob, boxes, mask, conf_thresh, nms_thr, top_k, max_det)
        return d, t, 0
    return traditional_nms(prob, boxes, mask, conf_thresh, nms_thr, max_det, max_size, cap)
