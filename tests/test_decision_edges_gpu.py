"""The detection tail's discrete decisions AT their knife edges, HIP kernels against the CPU oracle, bit for bit: IoU quotients equal to the NMS threshold
or one ulp from it through every site of the division-free predicate, special float keys through every top-k instance, the deterministic math on every
branch point, probabilities exactly on conf_thresh / score_thr, mask values within an ulp of 0.5.  The inputs come from tests/decision_cases.py;
tests/test_decision_cases_cpu.py proves on the CPU that they discriminate (the oracle's verdict per class, the opposite verdict of a naive predicate).

Which test reaches what:
  iou_exceeds() sites   nms_block            test_iou_windows_nms (nms_kernel n = 128, nms_big_kernel n = 1026), test_iou_windows_rpn[chip_wide False]
                                             (rpn_decode_nms_kernel), test_iou_windows_box_postprocess R = 40 (in-block box NMS)
                        nms_matrix_block     test_iou_windows_box_postprocess R = 140, chip_wide False
                        rpn_nms_matrix_kernel   test_iou_windows_rpn (chip_wide True, and isegmi_op_rpn_levels)
                        box_nms_matrix_kernel   test_iou_windows_box_postprocess R = 140, chip_wide True
  topk_kernel<NT, KCAP>  test_topk_special_keys, one parameter per instance (named there)
  the `!(uni > 0)` branch of iou_exceeds()   all four degenerate unions (0/0, negative, +inf, NaN) reach it through ffi.nms only, i.e. in nms_block.  The decode
                        paths (rpn_level, rpn_levels, box_postprocess) clip the 2e19 coordinates to the image first, so rpn_nms_matrix_kernel, box_nms_matrix_kernel,
                        nms_matrix_block and the in-kernel RPN path see the 0/0 and the negative union only (the other two pairs arrive as identical boxes).
Comparisons go through the bit patterns wherever a zero's sign or a NaN can occur."""
import functools

import numpy as np
import pytest

import decision_cases as dc
from oracle import ora

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
THRS = [0.7, 0.3, 0.5]
BIG_HW = 1 << 25   # image side for the decode paths: clipping is the identity on every window (widths up to 2^24)


@functools.lru_cache(maxsize=None)
def _cases(thr, plus_one):
    return dc.iou_window_cases(F32(thr), plus_one)


def _pair_set(thr, plus_one, n_pairs, keep=None, degenerate=False, skip=0):
    """n_pairs stacked pairs, the classes taking turns -> (boxes [2 n, 4] with A_i at 2 i and B_i at 2 i + 1, [class of pair i]).  keep: a filter on
    (pairs [m, 2, 4]) -> bool [m] (the decode paths take only pairs their box coder reproduces exactly); degenerate: the last four pairs are the
    degenerate-union ones (plain areas only); skip: start each class `skip` pairs further on (another draw for a second level)."""
    cases = _cases(thr, plus_one)
    pools = {}
    for c in dc.IOU_CLASSES:
        p = cases[c]
        if keep is not None and len(p):
            p = p[keep(p)]
        if len(p):
            pools[c] = np.roll(p, -(skip % len(p)), axis=0)
    deg = dc.degenerate_union_pairs() if degenerate else []
    want = n_pairs - len(deg)
    pairs, names, i = [], [], 0
    while len(pairs) < want:
        took = False
        for c, p in pools.items():
            if i < len(p) and len(pairs) < want:
                pairs.append(p[i]); names.append(c); took = True
        assert took, "not enough window pairs"
        i += 1
    st = dc.stack_pairs(np.stack(pairs))
    if deg:
        st = np.concatenate([st, np.array([[a, b] for _, a, b in deg], F32)])
        names += [n for n, _, _ in deg]
    return st.reshape(-1, 4), names


def _ranked_scores(n_pairs, hi=3.0, lo=-3.0):
    """logits / scores that rank A_i above B_i and pair i above pair i + 1: a strictly decreasing ramp over the 2 n boxes"""
    return np.linspace(hi, lo, 2 * n_pairs).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ 1. IoU windows
@pytest.mark.parametrize("n", [128, 1026])   # nms_kernel | nms_big_kernel (64 pairs + 898 far-away boxes)
@pytest.mark.parametrize("plus_one", [0, 1])
@pytest.mark.parametrize("thr", THRS)
def test_iou_windows_nms(ffi, thr, plus_one, n):
    boxes, names = _pair_set(thr, plus_one, 64, degenerate=not plus_one)
    scores = _ranked_scores(64, 2.0, 1.0)
    if n > len(boxes):
        m = n - len(boxes)
        far = np.zeros((m, 4), F32)
        far[:, 1] = 1e6 + 4 * np.arange(m); far[:, 3] = far[:, 1] + 1; far[:, 2] = 2
        boxes = np.concatenate([boxes, far]); scores = np.concatenate([scores, np.linspace(0.9, 0.1, m).astype(F32)])
    kept = {}
    for ge in (0, 1):
        got = ffi.nms(boxes[None], scores[None], thr, plus_one, ge)[0]
        ref = ora.nms(boxes, scores, thr, plus_one, ge)
        assert np.array_equal(got, ref), (ge, [names[i // 2] for i in np.setxor1d(got, ref) if i < 128])
        kept[ge] = len(ref)
    assert kept[1] < kept[0] < n   # `succ` pairs are suppressed either way, `exact` (and `above` / `below`) pairs only under >=


def _rows_found_in(out_boxes, in_boxes):
    """how many of the returned boxes are, bit for bit, input boxes: all of them when decoding and clipping were the identity (the four degenerate boxes
    with 1e19 coordinates are the exception: they are clipped to the image)"""
    return sum(bool((in_boxes == b).all(1).any()) for b in out_boxes)


def _rpn_decodes_exactly(pairs):
    flat = pairs.reshape(-1, 4)
    dec = ora.decode_boxes(flat, np.zeros_like(flat), (1.0, 1.0, 1.0, 1.0), float(BIG_HW), float(BIG_HW))
    return (dec.reshape(-1, 2, 4) == pairs).all((1, 2))


def _box_decodes_exactly(pairs):
    flat = pairs.reshape(-1, 4)
    dec = ora.decode_boxes(flat, np.zeros_like(flat), (10.0, 10.0, 5.0, 5.0), float(BIG_HW), float(BIG_HW))
    return (dec.reshape(-1, 2, 4) == pairs).all((1, 2))


@pytest.mark.parametrize("ge", [0, 1])
@pytest.mark.parametrize("plus_one", [0, 1])
@pytest.mark.parametrize("thr", THRS)
def test_iou_windows_rpn(ffi, thr, plus_one, ge):
    """The pairs are the ANCHORS of a 4 x 4 x 8 grid with all deltas zero (decoding and clipping are the identity: asserted on the oracle's boxes), the
    objectness ranks A_i above B_i; pre_nms = 300 admits the batched op.  Only pairs the box coder reproduces exactly take part: under plain areas that
    leaves out the 2^24-wide `exact` pairs of 0.7 / 0.3 (width + 1 is not an fp32 number) and keeps their 2-D ones with sides below 2^23; every class is
    there (asserted)."""
    flags = (1 if ge else 0) | (0 if plus_one else 2)
    A, pre, post = 8, 300, 300
    hw = np.array([[BIG_HW, BIG_HW]], np.int32)
    levels = []
    for skip in (0, 14):
        anchors, names = _pair_set(thr, plus_one, 64, keep=_rpn_decodes_exactly, degenerate=not plus_one, skip=skip)
        assert {"pred", "succ", "exact"} <= set(names) and (thr == 0.5 or {"above", "below"} <= set(names))
        head = np.zeros((1, 4, 4, A * 5), F32)
        head.reshape(16, A * 5)[:, :A] = _ranked_scores(64).reshape(16, A)
        levels.append((head, anchors, names))
    refs = []
    for head, anchors, names in levels:
        rb, rs = ora.rpn_level(head[0, ..., :A].reshape(-1), head[0, ..., A:].reshape(-1, 4), anchors, pre, post, thr, 0.0, float(BIG_HW), float(BIG_HW), flags)
        assert _rows_found_in(rb, anchors) >= len(rb) - (0 if plus_one else 4)
        assert 64 <= len(rs) < 128
        refs.append((rb, rs))
        for chip_wide in (True, False):
            (gb, gs), = ffi.rpn_level(head, anchors, hw, A, pre, post, nms_thr=thr, nms_flags=flags, chip_wide=chip_wide)
            assert np.array_equal(gs, rs) and np.array_equal(gb, rb), (chip_wide, len(gs), len(rs))
    got = ffi.rpn_levels([l[0] for l in levels], [l[1] for l in levels], hw, A, pre, post, nms_thr=thr, nms_flags=flags)
    for l, (rb, rs) in enumerate(refs):
        assert np.array_equal(got[l][0][1], rs) and np.array_equal(got[l][0][0], rb), l


@pytest.mark.parametrize("R", [140, 40])   # 140 candidates of one class: box_nms_matrix_kernel (chip_wide) | nms_matrix_block; 40: nms_block
@pytest.mark.parametrize("plus_one", [0, 1])
@pytest.mark.parametrize("thr", THRS)
def test_iou_windows_box_postprocess(ffi, thr, plus_one, R):
    props, names = _pair_set(thr, plus_one, R // 2, keep=_box_decodes_exactly, degenerate=not plus_one)
    assert {"pred", "succ", "exact"} <= set(names) and (thr == 0.5 or {"above", "below"} <= set(names))
    logits = np.zeros((1, R, 2), F32); logits[0, :, 1] = _ranked_scores(R // 2, 3.0, -1.0)   # every probability > 0.26 > score_thr
    p = ora.softmax(logits[0])[:, 1]
    assert (np.diff(p) < 0).all() and p.min() > 0.05
    regr = np.zeros((1, R, 8), F32)
    cnt, hw = np.array([R], np.int32), np.array([[BIG_HW, BIG_HW]], np.int32)
    for ge in (0, 1):
        flags = ge | (0 if plus_one else 2)
        rb, rs, rl = ora.box_postprocess(logits[0], regr[0], props, float(BIG_HW), float(BIG_HW), nms_thr=thr, det_per_img=R, nms_flags=flags, cap=R)
        assert R // 2 <= len(rs) < R
        assert _rows_found_in(rb, props) >= len(rb) - (0 if plus_one else 4)   # decoded == proposal
        for chip_wide in (True, False):
            (gb, gs, gl), = ffi.box_postprocess(logits, regr, props[None], cnt, hw, nms_thr=thr, det_per_img=R, nms_flags=flags, chip_wide=chip_wide)
            assert np.array_equal(gl, rl) and np.array_equal(gs, rs) and np.array_equal(gb, rb), (ge, chip_wide, len(gs), len(rs))


# ------------------------------------------------------------------------------------------------------------------ 2. Yolact fast NMS
@pytest.mark.parametrize("thr", THRS)
def test_iou_windows_yolact_fast_nms(ffi, thr):
    """jaccard() divides; `!(o <= thr)` keeps a box at o == thr and drops it at NaN.  The windows are the plain-area ones, realised as priors whose decoded
    boxes (loc = 0) are the strips: only pairs that ora.yolact_decode reproduces exactly are used.  40 pairs + the 0/0 pair = 82 priors <= max_det."""
    def keep(pairs):
        pri = np.stack([(pairs[..., 0] + pairs[..., 2]) / 2, (pairs[..., 1] + pairs[..., 3]) / 2, pairs[..., 2] - pairs[..., 0], pairs[..., 3] - pairs[..., 1]], -1)
        dec = ora.yolact_decode(np.zeros((pri.size // 4, 4), F32), pri.reshape(-1, 4).astype(F32))
        return (dec.reshape(-1, 2, 4) == pairs).all((1, 2))
    boxes, names = _pair_set(thr, 0, 40, keep=keep)
    assert {"pred", "succ"} <= set(names) and (thr == 0.5 or {"above", "below"} <= set(names))
    boxes = np.concatenate([boxes, np.array([[5, 2e6, 5, 2e6], [5, 2e6, 5, 2e6]], F32)])    # 0 / 0: NaN drops the second one
    P = len(boxes)
    priors = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2, boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], 1).astype(F32)
    loc = np.zeros((1, P, 4), F32)
    conf = np.zeros((1, P, 2), F32); conf[0, :, 1] = np.linspace(4.0, 0.0, P)
    mask = np.random.default_rng(3).standard_normal((1, P, 32)).astype(F32)
    dec = ora.yolact_decode(loc[0], priors)
    assert np.array_equal(dec, boxes)
    ref = ora.yolact_detect(ora.softmax(conf[0]), dec, mask[0], nms_thr=thr)
    got, gboxes = ffi.yolact_detect(conf, loc, mask, priors, nms_thresh=thr)
    assert np.array_equal(gboxes[0], dec)
    assert 41 <= len(ref["score"]) < P and P - 1 not in ref["prior"] and P - 2 in ref["prior"]
    for key in ("prior", "cls", "score", "box", "mask"):
        assert np.array_equal(got[0][key], ref[key]), key


# ------------------------------------------------------------------------------------------------------------------ 3. top-k keys
def _check_topk(vals, idx, cnt, keys, k, limit=None, rows_per_limit=1):
    """against ora.topk row by row: indices exactly; values by bit pattern, except that a selected zero comes back as +0 whatever its sign (the documented
    contract of isegmi_op_topk: the value is rebuilt from the sort key, in which the two zeros are one)"""
    for r in range(keys.shape[0]):
        kk = k if limit is None else min(k, int(limit[r // rows_per_limit]))
        s, i = ora.topk(keys[r], kk) if kk > 0 else (np.zeros(0, F32), np.zeros(0, np.int32))
        assert cnt[r] == len(s), (r, cnt[r], len(s))
        assert np.array_equal(idx[r, : cnt[r]], i), (r, np.nonzero(idx[r, : cnt[r]] != i)[0][:8])
        v, nz = vals[r, : cnt[r]], s != 0
        assert np.array_equal(dc.bits(v[nz]), dc.bits(s[nz])) and np.array_equal(dc.bits(v[~nz]), np.zeros((~nz).sum(), U32)), r


TOPK_SHAPES = [   # rows, n, ks (KCAP - 1, KCAP, and KCAP + 1 of the instance below), two-level slice border -- and the topk_launch_ws instance the shape reaches
    (6, 300, (100, 127, 128), None),                # topk_kernel<256, 128>
    (6, 9000, (100, 127, 128), None),               # topk_kernel<1024, 128>   (n > 8192, rows < 256)
    (6, 300, (200, 129, 255, 256), None),           # topk_kernel<256, 256>
    (6, 9000, (200, 129, 255, 256), None),          # topk_kernel<1024, 256>
    (64, 2000, (600, 257, 1023, 1024), None),       # topk_kernel<256, 1024>  (rows >= 64, n <= 16384)
    (6, 2000, (600, 257, 1023, 1024), None),        # topk_kernel<1024, 1024> (rows < 64)
    (6, 40000, (300, 257, 1023, 1024), 10000),      # two levels of topk_kernel<1024, 1024>: 4 slices of 10 000 keys, one row's zero-valued cut on the first border
    (6, 9000, (2000, 1025, 8191, 8192), None),      # topk_kernel<1024, 8192>
]
LIMIT_ROWS = 12   # rows of the `limit` runs where the shape has fewer: four limit groups of rows_per_limit = 3 (no dispatch rule of topk_launch_ws moves below 64 rows)


def _key_rows(rows, n, k, border):
    """[rows, n]: the key sets of topk_key_sets(n, k) taking turns (6 of them with a border, 5 without)"""
    sets = dc.topk_key_sets(n, k, border=border)
    return np.stack([sets[r % len(sets)][1] for r in range(rows)])


@pytest.mark.parametrize("rows,n,ks,border", TOPK_SHAPES, ids=["256x128", "1024x128", "256x256", "1024x256", "256x1024", "1024x1024", "two-level", "1024x8192"])
def test_topk_special_keys(ffi, rows, n, ks, border):
    """+-0, subnormals, +-FLT_MAX, +-inf with the cut on a zero, on -inf, on a subnormal, every key set in every launch: k at and around each instance's
    capacity; row_stride = n + 5 with +inf in the gaps between the rows; `limit` with rows_per_limit 1 and 3, every shape seeing the limits 0, 1, k / 2 and
    k + 7 (above k) in both orders.  (A limit switches the two-level form off: that shape's limit runs are one-level <1024, 1024> launches over 40 000 keys.)"""
    for k in ks:
        keys = _key_rows(rows, n, k, border)
        _check_topk(*ffi.topk(keys, k), keys, k)
    k = ks[0]
    keys = _key_rows(max(rows, LIMIT_ROWS), n, k, border)
    _check_topk(*ffi.topk(keys[:rows], k, row_stride=n + 5), keys[:rows], k)
    for rpl in (1, 3):
        limit = np.resize(np.array([0, k + 7, k // 2, 1], np.int32), -(-len(keys) // rpl))
        assert {0, 1, k // 2, k + 7} <= set(limit.tolist())
        _check_topk(*ffi.topk(keys, k, limit=limit, rows_per_limit=rpl), keys, k, limit, rpl)
        _check_topk(*ffi.topk(keys, k, limit=limit[::-1].copy(), rows_per_limit=rpl, row_stride=n + 5), keys, k, limit[::-1], rpl)


def test_topk_and_nms_minus_zero_before_plus_zero(ffi):
    """The simplest input on which a bit-pattern order and the contract differ: keys [-0, +0], k = 1 -> index 0 (equal keys, lower index first)."""
    keys = np.array([[-0.0, 0.0]], F32)
    vals, idx, cnt = ffi.topk(keys, 1)
    assert cnt[0] == 1 and idx[0, 0] == 0 == ora.topk(keys[0], 1)[1][0] and vals[0, 0] == 0
    boxes = np.array([[[0, 0, 9, 9], [100, 100, 120, 120]]], F32)
    assert list(ffi.nms(boxes, keys, 0.5)[0]) == [0, 1] == list(ora.nms(boxes[0], keys[0], 0.5))


# ------------------------------------------------------------------------------------------------------------------ 4. NMS visiting order
@pytest.mark.parametrize("n", [200, 1024, 1030])
def test_nms_visiting_order_with_zero_scores(ffi, n):
    """scores of mixed +-0 and equal positives on clustered boxes: the visiting order (score descending, zeros equal, index ascending) decides which box of
    a cluster survives, and the keep list is in that order"""
    rng = np.random.default_rng(n)
    c = rng.uniform(0, 1, (n, 2)) * [600, 400]
    c[n // 2:] = c[: n - n // 2] + rng.normal(0, 4, (n - n // 2, 2))
    wh = rng.uniform(20, 90, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    scores = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 0.5, 0.25], F32), n)
    for thr, plus_one, ge in ((0.5, 1, 0), (0.3, 0, 1)):
        got = ffi.nms(boxes[None], scores[None], thr, plus_one, ge)[0]
        ref = ora.nms(boxes, scores, thr, plus_one, ge)
        assert np.array_equal(got, ref)
        assert 10 < len(ref) < n and (scores[ref] == 0).sum() > 5


# ------------------------------------------------------------------------------------------------------------------ 5. detmath
@pytest.mark.parametrize("fn", [dc.EXP, dc.SIGMOID, dc.TANH, dc.LOG2], ids=["exp", "sigmoid", "tanh", "log2"])
def test_detmath_on_every_branch_point(ffi, fn):
    """Every result as uint32, NaN results included: both sides hand a NaN input on quieted, payload kept (exp and tanh with its sign, sigmoid with the
    sign flipped by its exp(-x)); 12 474 of the patterns are NaNs."""
    x = dc.detmath_inputs(fn).view(F32)
    got, ref = dc.bits(ffi.map_f32(x, fn)), dc.bits(ora.map_f32(x, fn))
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, (bad.size, [(hex(v), hex(a), hex(b)) for v, a, b in zip(dc.bits(x[bad[:8]]), got[bad[:8]], ref[bad[:8]])])
    assert fn == dc.LOG2 or np.isnan(ref.view(F32)).sum() > 1000   # (NaN in, NaN out; log2 sees positive normal inputs only)


# ------------------------------------------------------------------------------------------------------------------ 6. thresholds reached exactly
def _disjoint_priors(P):
    return np.stack([0.1 + 0.13 * np.arange(P), np.full(P, 0.5), np.full(P, 0.1), np.full(P, 0.1)], 1).astype(F32)


def test_conf_thresh_reached_exactly_yolact(ffi):
    """81 classes: priors whose best foreground probability is pred(0.05f), 0.05f (both dropped: the test is >) and succ(0.05f) (kept); three more that pass on
    a dominant class and carry a second class at pred / on / succ, which only second_threshold looks at.  2 classes: the two reachable probabilities
    next to 0.05f (threshold_logits' docstring: 0.05f itself is not reachable there)."""
    thr = F32(0.05)
    first = dc.threshold_logits(ora.softmax, thr, 81, cls=80)
    second = dc.threshold_logits(ora.softmax, thr, 81, cls=5, also=(3, 2.0))
    conf = np.stack([first["pred"], first["on"], first["succ"], second["pred"], second["on"], second["succ"]])[None]
    P = conf.shape[1]
    priors, loc = _disjoint_priors(P), np.zeros((1, P, 4), F32)
    mask = np.random.default_rng(4).standard_normal((1, P, 32)).astype(F32)
    dec = ora.yolact_decode(loc[0], priors)
    for st in (0, 1):
        ref = ora.yolact_detect(ora.softmax(conf[0]), dec, mask[0], second_threshold=st)
        got, _ = ffi.yolact_detect(conf, loc, mask, priors, second_threshold=st)
        for key in ("prior", "cls", "score", "box", "mask"):
            assert np.array_equal(got[0][key], ref[key]), (st, key)
        assert 0 not in ref["prior"] and 1 not in ref["prior"] and 2 in ref["prior"]
    assert sorted(zip(ref["prior"].tolist(), ref["cls"].tolist())) == [(2, 79), (3, 2), (4, 2), (5, 2), (5, 4)]   # second_threshold: class 5 of prior 5 only
    two = dc.threshold_logits(ora.softmax, thr, 2)
    conf = np.stack([two["below"], two["above"]])[None]
    priors, loc, mask = _disjoint_priors(2), np.zeros((1, 2, 4), F32), mask[:, :2]
    for st in (0, 1):
        ref = ora.yolact_detect(ora.softmax(conf[0]), ora.yolact_decode(loc[0], priors), mask[0], second_threshold=st)
        got, _ = ffi.yolact_detect(conf, loc, mask, priors, second_threshold=st)
        assert list(ref["prior"]) == [1] == list(got[0]["prior"]) and np.array_equal(got[0]["score"], ref["score"])


def test_score_thr_reached_exactly_box_postprocess(ffi):
    thr = F32(0.05)
    props = np.array([[10 + 60 * i, 10, 50 + 60 * i, 40] for i in range(3)], F32)
    hw = np.array([[100, 300]], np.int32)
    rows = dc.threshold_logits(ora.softmax, thr, 81, cls=80)
    two = dc.threshold_logits(ora.softmax, thr, 2)
    for logits, keep in ((np.stack([rows["pred"], rows["on"], rows["succ"]]), 2), (np.stack([two["below"], two["below"], two["above"]]), 2)):
        ncls = logits.shape[1]
        regr = np.zeros((1, 3, 4 * ncls), F32)
        rb, rs, rl = ora.box_postprocess(logits, regr[0], props, 300.0, 100.0)
        assert len(rs) == 1 and np.array_equal(rb[0], props[keep]) and rs[0] > thr
        for chip_wide in (True, False):
            (gb, gs, gl), = ffi.box_postprocess(logits[None], regr, props[None], np.array([3], np.int32), hw, chip_wide=chip_wide)
            assert np.array_equal(gl, rl) and np.array_equal(gs, rs) and np.array_equal(gb, rb)


# ------------------------------------------------------------------------------------------------------------------ 7. masks on the 0.5 edge
def _paste_boxes(h, w):
    return np.array([
        [0.3, 0.2, w * 0.7 + 0.4, h * 0.6 + 0.3],            # fractional corners
        [0, 0, w - 1, h - 1],                                # the whole image
        [min(2, w - 1), min(1, h - 1), min(2, w - 1), min(1, h - 1)],   # one pixel
        [-60.5, 0, -20.25, h - 1],                           # wholly outside: left
        [w + 20.5, 0, w + 60, h - 1],                        # right
        [0, -70, w - 1, -30.5],                              # top
        [0, h + 30.5, w - 1, h + 70],                        # bottom
        [w + 25.5, h + 31.25, w + 60, h + 75],               # both axes at once: window width and height both negative
        [w * 0.8, h * 0.7, w * 0.2, h * 0.1],                # reversed corners
        [-5e5, 0.25, 5e5, h - 0.5],                          # 10^6 wide
    ], F32)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 1), (3, 2), (7, 3), (9, 5), (64, 67), (203, 317)])
def test_paste_masks_on_the_knife_edge(ffi, h, w):
    """Mask values within an ulp of thr = 0.5 (every interior blend is a knife-edge decision), planes that start off a 4-byte boundary and are narrower than a
    word (the tail store path), and the degenerate windows: wholly outside on each side and on both axes, reversed, a million pixels wide."""
    rng = np.random.default_rng(h * 1000 + w)
    boxes = np.stack([_paste_boxes(h, w), _paste_boxes(h, w)[::-1]])
    N, K = boxes.shape[:2]
    masks = dc.knife_edge_masks((N, K, 28, 28), rng)
    cnt = np.array([K, 6], np.int32)
    out = ffi.paste_masks(masks, boxes, cnt, h, w, 0.5)
    total = 0
    for n in range(N):
        ref = ora.paste_masks(masks[n, : cnt[n]], boxes[n, : cnt[n]], h, w, 0.5)
        assert np.array_equal(out[n, : cnt[n]], ref), (n, np.nonzero((out[n, : cnt[n]] != ref).reshape(cnt[n], -1).any(1))[0])
        assert not out[n, cnt[n]:].any()
        total += int(ref.sum())
    assert h * w < 20 or 0 < total < N * K * h * w


@functools.lru_cache(maxsize=None)
def _knife_edge_prototypes():
    """proto [1, 138, 138, 32], coeffs [1, 6, 32], boxes [1, 6, 4]: detection d reads channels 5 d .. 5 d + 4 (its other coefficients are 0: the chain's other
    27 steps add +-0) as r1 c1 - r1 c1 + r2 c2 - r2 c2 + t: two products that cancel up to their rounding error (a few 1e-9) and a logit t at the centre
    of the interval on which the oracle's sigmoid is 0.5 - 2^-24, 0.5 or succ(0.5).  Pixels whose
    residue pushed the sigmoid off those three values (found on the oracle) fall back to r = a power of two: exact products, exact cancellation.
    The steps of the sigmoid are ~1e-7 wide in the logit, so the dot product is NOT on an edge here (another association of the chain would move the
    residue by 1e-9 and the sigmoid not at all): what sits on the edge is the upsampling blend of these values and its `> 0.5`."""
    rng = np.random.default_rng(77)
    PH = PW = 138
    grid = (np.arange(-4000, 4001) * 2.0 ** -31).astype(F32)
    sg = ora.map_f32(grid, dc.SIGMOID)
    # the oracle's sigmoid = 1 / (1 + exp(-x)) cannot return pred(0.5): 1 + e has 2^-22 spacing above 2, so just below one half its values lie
    # 2^-24 = two ulps apart.  The nearest value below 0.5 it does return, 0.5 - 2^-24, stands in.
    targets = np.array([0.5 - 2.0 ** -24, 0.5, dc.f32_succ(0.5)], F32)
    assert not (sg == dc.f32_pred(0.5)).any()
    t = np.array([grid[np.nonzero(sg == v)[0][len(np.nonzero(sg == v)[0]) // 2]] for v in targets], F32)
    K = 6
    proto = np.zeros((PH, PW, 32), F32); coeffs = np.zeros((K, 32), F32)
    which = rng.integers(0, 3, (K, PH, PW))
    for d in range(K):
        c1, c2 = rng.uniform(0.1, 0.5, 2).astype(F32) * rng.choice([-1, 1], 2).astype(F32)
        coeffs[d, 5 * d: 5 * d + 5] = [c1, -c1, c2, -c2, 1.0]
        r = rng.uniform(0.05, 0.3, (2, PH, PW)).astype(F32)
        proto[..., 5 * d] = proto[..., 5 * d + 1] = r[0]
        proto[..., 5 * d + 2] = proto[..., 5 * d + 3] = r[1]
        proto[..., 5 * d + 4] = t[which[d]]
    c = np.array([[0.5, 0.5], [0.3, 0.6], [0.7, 0.2], [0.5, 0.5], [0.1, 0.9], [0.02, 0.02]]); s = np.array([[1.2, 1.2], [0.4, 0.5], [0.3, 0.3], [0.9, 0.1], [0.3, 0.3], [0.03, 0.03]])
    boxes = np.concatenate([c - s / 2, c + s / 2], 1).astype(F32)
    boxes[2] = boxes[2, [2, 3, 0, 1]]   # swapped corners
    whole = np.tile(np.array([[-1.0, -1.0, 2.0, 2.0]], F32), (K, 1))
    lo = ora.yolact_proto_masks(proto, coeffs, whole)
    for d in range(K):
        bad = ~np.isin(lo[d], targets)
        proto[..., 5 * d: 5 * d + 4][bad] = (2.0 ** -rng.integers(1, 5, (int(bad.sum()), 1))).astype(F32)
    lo = ora.yolact_proto_masks(proto, coeffs, whole)
    return proto[None], coeffs[None], boxes[None], lo, targets


@pytest.mark.parametrize("h,w", [(1, 1), (3, 1000), (1000, 3), (138, 138), (69, 277)])
def test_yolact_masks_on_the_knife_edge(ffi, h, w):
    proto, coeffs, boxes, lo, targets = _knife_edge_prototypes()
    for d in range(lo.shape[0]):
        assert np.isin(lo[d], targets).all() and all((lo[d] == v).mean() > 0.2 for v in targets), d   # nothing but the three knife-edge values
    cnt = np.array([6], np.int32)
    masks, ib = ffi.yolact_masks(proto, coeffs, boxes, cnt, h, w)
    ref_m, ref_b = ora.yolact_masks(proto[0], coeffs[0], boxes[0], h, w)
    assert np.array_equal(masks[0], ref_m) and np.array_equal(ib[0], ref_b)
    assert h * w < 10 or 0 < ref_m.sum() < ref_m.size
