"""isegmi_op_bbox_aug_candidates, the merge over its pool and isegmi_op_preprocess_u8_flip, op by op and bit for bit against tests/bbox_aug_ref.py
(DESIGN.md 23).  Shapes: rows around the wave (63, 64, 65), the place kernel's 16-row blocks and the largest R; class counts 2, 81 and 256 (one, two
and four 64-lane passes over a row)."""
import functools

import numpy as np
import pytest

import bbox_aug_cases as bc
import bbox_aug_ref as br
from decision_cases import threshold_logits
from oracle import ora

pytestmark = pytest.mark.gpu
F32 = np.float32
ROWS = (1, 63, 64, 65, 1000, 1024)
CLASSES = (2, 81, 256)
PATTERNS = ("all", "none", "alternate")
RATIOS = ((F32(1.0), F32(1.0)), (F32(2.0), F32(2.0)), bc.RATIO_23)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def ref_views(views, cap, entry=None):
    """-> per image ((boxes, scores, labels) of the pool, total) after the views (each: dict of generated() form + hflip, ratios)."""
    out = []
    N = views[0]["logits"].shape[0]
    for n in range(N):
        cands = [br.candidates(v["logits"][n], v["regr"][n], v["props"][n], v["cnt"][n], v["hw"][n], v.get("hflip", False), v.get("ratios", RATIOS[0]),
                               v["thr"], v["agnostic"]) for v in views]
        e = None if entry is None else entry[n]
        pooled, total = br.pool(cands, cap, e)
        out.append((pooled, total))
    return out


def run_view(ffi, pool, v):
    N = v["logits"].shape[0]
    ffi.bbox_aug_candidates(pool, v["logits"], v["regr"], v["props"], v["cnt"], v["hw"], v.get("hflip", False),
                            np.tile(np.array(v.get("ratios", RATIOS[0]), F32), (N, 1)), v["thr"], v["agnostic"])


def assert_pool(pool, ref, what=""):
    B, S, Lb, cnt, total = pool.numpy()
    for n, ((rb, rs, rl), rtotal) in enumerate(ref):
        print(what, "image", n, "pool count", int(cnt[n]), "total", int(total[n]), "reference", len(rs), rtotal)
        assert int(total[n]) == rtotal and int(cnt[n]) == len(rs) == min(pool.cap, rtotal), (what, n)
        c = len(rs)
        assert np.array_equal(Lb[n, :c], rl), (what, n, "labels")
        assert np.array_equal(bits(S[n, :c]), bits(rs)), (what, n, "scores")
        assert np.array_equal(bits(B[n, :c]), bits(rb)), (what, n, "boxes")
        # slots at or past the count keep the poison they were created with: nothing is written there
        assert (bits(S[n, c:]) == 0xFFFFFFFF).all() and (Lb[n, c:] == -1).all() and (bits(B[n, c:]) == 0xFFFFFFFF).all(), (what, n, "past the count")


@pytest.mark.parametrize("ncls", CLASSES)
@pytest.mark.parametrize("R", ROWS)
def test_candidates_rows_classes_patterns(ffi, R, ncls):
    """Every pass pattern at every (R, ncls), N = 4 with proposal counts 0, 1, R - 1, R and NaN rows past them; cls_agnostic, the flip and the ratio
    rotate over the cases.  The pool is 8192 slots: "all" at R >= 63 x 81 classes overflows it, and then holds the first 8192 in (proposal, class) order."""
    k = ROWS.index(R) + CLASSES.index(ncls)
    for pi, pattern in enumerate(PATTERNS):
        v = dict(bc.generated(R, ncls, pattern, agnostic=(k + pi) % 2 == 1), hflip=(k + pi) % 3 != 0, ratios=RATIOS[(k + pi) % 3])
        pool = ffi.BBoxAugPool(4, 8192)
        run_view(ffi, pool, v)
        assert_pool(pool, ref_views([v], 8192), "%s R=%d ncls=%d" % (pattern, R, ncls))


def test_two_runs_give_identical_bytes(ffi):
    v = dict(bc.generated(1000, 81, "alternate", False), hflip=True, ratios=bc.RATIO_23)
    outs = []
    for _ in range(2):
        pool = ffi.BBoxAugPool(4, 8192)
        run_view(ffi, pool, v)
        outs.append([a.tobytes() for a in pool.numpy()])
    assert outs[0] == outs[1]


@functools.lru_cache(maxsize=None)
def threshold_view():
    """Rows whose class-2 probability is exactly pred(0.05), 0.05 and succ(0.05) (ncls 5), then the same three for class 4: only the succ rows pass."""
    rows = [threshold_logits(ora.softmax, 0.05, 5, cls=c)[k] for c in (2, 4) for k in ("pred", "on", "succ")]
    logits = np.stack(rows)[None].astype(F32)
    rng = np.random.default_rng(3)
    return dict(logits=logits, regr=rng.normal(0, 0.5, (1, 6, 20)).astype(F32), props=bc._props(rng, 6, 300.0, 200.0)[None], cnt=np.array([6], np.int32),
                hw=np.array([[200, 300]], np.int32), thr=0.05, agnostic=False, ncls=5)


def test_score_exactly_at_the_threshold_does_not_pass(ffi):
    v = threshold_view()
    pool = ffi.BBoxAugPool(1, 64)
    run_view(ffi, pool, v)
    ref = ref_views([v], 64)
    assert_pool(pool, ref, "threshold")
    p = ora.softmax(v["logits"][0])
    assert p[1, 2] == F32(0.05) and p[4, 4] == F32(0.05)
    (_, rs, rl), total = ref[0]
    assert total == 2 and list(rl) == [2, 4] and (rs > F32(0.05)).all()


@pytest.mark.parametrize("entry", [0, 1, 63])
def test_pool_entered_at_a_count_and_the_overflow_edge(ffi, entry):
    """A 64-slot pool entered at 0, 1 and cap - 1 entries: the view's candidates go behind them, the entries stay, and the pool keeps the first 64.  The view
    is cut to exactly as many candidates as reach total == cap (no overflow) and then one more (total == cap + 1: the first cap are kept)."""
    cap = 64
    g = bc.generated(65, 81, "alternate", False)
    rng = np.random.default_rng(entry)
    eb = rng.uniform(0, 100, (1, entry, 4)).astype(F32); es = rng.uniform(0.1, 1, (1, entry)).astype(F32); el = rng.integers(1, 81, (1, entry)).astype(np.int32)
    for extra in (0, 1):
        # image 3 of the generated case (all 65 rows live, about 40 passing classes a row), cut to exactly `want` candidates: in the row the cut falls
        # into, the candidates behind it drop to the level of the failing classes (the survivors only gain); every later row gets a dominant background
        want = cap - entry + extra
        logits = g["logits"][3:4].copy()
        ok = ora.softmax(logits[0]) > F32(g["thr"]); ok[:, 0] = False
        flat = np.flatnonzero(ok.ravel())
        cut_row = flat[want] // 81
        if flat[want - 1] // 81 != cut_row:      # the cut falls between two rows
            cut_row -= 1
        for f in flat[want:]:
            if f // 81 == cut_row:
                logits[0, cut_row, f % 81] = F32(-20.0)
        logits[0, cut_row + 1:, 0] = F32(20.0)
        v = dict(logits=logits, regr=g["regr"][3:4], props=g["props"][3:4], cnt=g["cnt"][3:4], hw=g["hw"][3:4], thr=g["thr"], agnostic=False)
        pool = ffi.BBoxAugPool(1, cap, cnt=[entry])
        if entry:   # the entries alone; every other slot keeps its poison
            for buf, arr in ((pool.boxes, eb), (pool.scores, es), (pool.labels, el)):
                ffi.check(ffi.lib().isegmi_h2d(buf.ptr, np.ascontiguousarray(arr).ctypes.data, arr.nbytes))
        run_view(ffi, pool, v)
        ref = ref_views([v], cap, entry=[(eb[0], es[0], el[0])])
        assert ref[0][1] == cap + extra
        assert_pool(pool, ref, "entry %d extra %d" % (entry, extra))


def test_two_views_append_view_major_with_different_counts(ffi):
    """N = 2 images with different counts, two views (the second flipped, at ratio 800 / 1200): view 1's candidates sit behind view 0's per image."""
    g0, g1 = bc.generated(63, 81, "alternate", False), bc.generated(65, 81, "alternate", True)
    pick = lambda g, idx: {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    v0 = dict(pick(g0, [2, 3]))
    v1 = dict(pick(g1, [3, 1]), hflip=True, ratios=bc.RATIO_23)
    pool = ffi.BBoxAugPool(2, 8192)
    run_view(ffi, pool, v0)
    run_view(ffi, pool, v1)
    ref = ref_views([v0, v1], 8192)
    assert ref[0][1] != ref[1][1]
    assert_pool(pool, ref, "two views")


@pytest.mark.parametrize("w_view", [100, 101])
@pytest.mark.parametrize("ratio", RATIOS)
def test_flip_at_the_borders(ffi, w_view, ratio):
    """Odd and even view widths, boxes touching the left border, the right border and both, at every ratio; against the reference and, for the boxes
    that need no decode (zero deltas), against the closed form x1' = w - 1 - x2 on integers."""
    c = bc.border_view(w_view)
    v = dict(logits=c["logits"][None], regr=c["regr"][None], props=c["props"][None], cnt=np.array([5], np.int32), hw=np.array([c["image_hw"]], np.int32),
             thr=0.05, agnostic=False, hflip=True, ratios=ratio)
    pool = ffi.BBoxAugPool(1, 64)
    run_view(ffi, pool, v)
    assert_pool(pool, ref_views([v], 64), "border w=%d" % w_view)
    B = pool.numpy()[0][0]
    w = float(w_view)
    assert np.array_equal(B[0], np.array([w - 1 - 20, 5, w - 1, 30], F32) * np.array([ratio[0], ratio[1]] * 2, F32))   # left border -> right border
    assert np.array_equal(B[1], np.array([0, 8, 20, 40], F32) * np.array([ratio[0], ratio[1]] * 2, F32))            # right border -> left border
    assert B[2][0] == 0 and B[2][2] == F32(w - 1) * ratio[0] and B[4][0] == 0 and B[4][2] == F32(w - 1) * ratio[0]    # both borders, and the clipped box


@pytest.mark.parametrize("flags", [0, 4])
def test_identity_view_and_merge_equal_box_postprocess(ffi, flags):
    """R = 300, ncls = 5, about 40 % of the (proposal, class) pairs above the threshold: candidates + merge of the identity view alone give what
    isegmi_op_box_postprocess gives on the same inputs, under both output orders (score order, ISEGMI_NMS_INDEX_ORDER)."""
    rng = np.random.default_rng(300)
    R, ncls = 300, 5
    logits = (rng.normal(0, 1.0, (1, R, ncls)) * 4.0).astype(F32)   # scaled so that about 40 % pass
    frac = float((ora.softmax(logits[0])[:, 1:] > F32(0.05)).mean())
    print("share of (proposal, class) pairs above 0.05:", frac)
    assert 0.35 < frac < 0.45
    hw = np.array([[400, 600]], np.int32)
    c = rng.uniform(40, 360, (24, 2))
    ctr = c[rng.integers(0, 24, R)] + rng.normal(0, 8.0, (R, 2))
    wh = rng.uniform(30, 120, (R, 2))
    props = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F32)[None]
    regr = rng.normal(0, 0.5, (1, R, 4 * ncls)).astype(F32)
    cnt = np.array([R], np.int32)
    want = ffi.box_postprocess(logits, regr, props, cnt, hw, 0.05, 0.5, 100, flags)[0]
    v = dict(logits=logits, regr=regr, props=props, cnt=cnt, hw=hw, thr=0.05, agnostic=False)
    pool = ffi.BBoxAugPool(1, 2048)
    run_view(ffi, pool, v)
    got = ffi.bbox_aug_merge(pool, ncls, 0.5, 100, 100, flags)[0]
    ref = br.merge(ref_views([v], 2048)[0][0], ncls, 0.5, 100, 100, flags)
    assert len(want[1]) == 100   # the kth-value cut is exercised
    for a, b, r in zip(got, want, ref):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(r))


def test_bad_sizes_are_refused_before_any_launch(ffi):
    g = bc.generated(1, 2, "all", False)
    for kw, word in ((dict(R=1025), "R <= 1024"), (dict(R=0), "R <= 1024"), (dict(ncls=257), "ncls <= 256"), (dict(ncls=1), "ncls <= 256"),
                     (dict(cap=0), "cap <= 8192"), (dict(cap=8193), "cap <= 8192")):
        pool = ffi.BBoxAugPool(4, 8)
        with pytest.raises(ffi.IsegmiError, match=word):
            ffi.bbox_aug_candidates(pool, g["logits"], g["regr"], g["props"], g["cnt"], g["hw"], **kw)
        B, S, Lb, cnt, total = pool.numpy()
        assert (cnt == 0).all() and (total == 0).all() and (Lb == -1).all()
    assert ffi.lib().isegmi_op_bbox_aug_workspace(1, 1025) == -1 and ffi.lib().isegmi_op_bbox_aug_workspace(0, 8) == -1


@pytest.mark.parametrize("w", [37, 40])
@pytest.mark.parametrize("resize", [False, True])
def test_preprocess_flip_equals_the_plain_op_on_a_flipped_copy(ffi, w, resize):
    """Odd and even widths, narrower than the padded canvas (w < Wpad: the mirror image stays at the left edge, the padding right and bottom), with and
    without a resize; and hflip = 0 is the plain op."""
    rng = np.random.default_rng(w)
    im = rng.integers(0, 256, (2, 29, w, 3), dtype=np.uint8)
    ho, wo = (45, w + 11) if resize else (29, w)
    Hp, Wp = 64, 64
    mean = (102.9801, 115.9465, 122.7717)
    want = ffi.preprocess_u8(np.ascontiguousarray(im[:, :, ::-1]), ho, wo, Hp, Wp, mean, (1, 1, 1), False)
    got = ffi.preprocess_u8_flip(im, ho, wo, Hp, Wp, mean, (1, 1, 1), False, True)
    assert np.array_equal(bits(got), bits(want))
    assert not got[:, :, wo:].any() and not got[:, ho:].any() and got[:, :ho, :wo].any()
    assert np.array_equal(bits(ffi.preprocess_u8_flip(im, ho, wo, Hp, Wp, mean, (1, 1, 1), False, False)), bits(ffi.preprocess_u8(im, ho, wo, Hp, Wp, mean, (1, 1, 1), False)))
