"""The generators of tests/decision_cases.py discriminate (so that a green tests/test_decision_edges_gpu.py means something), and the oracle they are
judged by is itself checked against independent references at the same inputs: numpy's stable sort for ora.topk, float64 numpy for the oracle's math."""
import numpy as np
import pytest

import decision_cases as dc
from oracle import ora

F32, U32 = np.float32, np.uint32
THRS = [F32(0.7), F32(0.3)]
FLOOR = 32   # cases per class, per threshold and plus_one


def _oracle_suppressed(pairs, thr, plus_one, ge):
    """ora.nms on the stacked pairs (A_i scored above B_i, only A_i and B_i overlap) -> bool [n]: B_i suppressed."""
    st = dc.stack_pairs(pairs)
    n = len(st)
    boxes = st.reshape(2 * n, 4)
    scores = np.empty(2 * n, F32)
    scores[0::2] = 2.0 - np.arange(n) / (2.0 * n); scores[1::2] = 1.0 - np.arange(n) / (2.0 * n)
    keep = ora.nms(boxes, scores, thr, plus_one, ge)
    kept = np.zeros(2 * n, bool); kept[keep] = True
    assert kept[0::2].all()
    return ~kept[1::2], st


EXPECT = {  # class -> (suppressed under >, suppressed under >=)
    "above": (False, True), "below": (False, True), "pred": (False, False), "succ": (True, True), "exact": (False, True)}


@pytest.mark.parametrize("plus_one", [0, 1])
@pytest.mark.parametrize("thr", THRS)
def test_iou_windows_discriminate(thr, plus_one):
    """Every class holds >= 32 pairs; the oracle's division gives the verdict the class predicts; the naive `inter > thr * uni` (exact product: the real
    quotient against thr) gives the OPPOSITE verdict on every on-from-above pair under > and on every on-from-below pair under >=; the midpoint predicate as
    iou_exceeds() writes it agrees with the oracle on every pair.  (The naive predicate with the product rounded to fp32 is wrong elsewhere: thr * uni is
    within a quarter of inter in both `on` classes and rounds ONTO it, so it agrees there and fails one ulp out; it must be wrong somewhere too.)"""
    cases = dc.iou_window_cases(thr, plus_one)
    fp32_naive_wrong = 0
    for cls in dc.IOU_CLASSES:
        pairs = cases[cls]
        assert len(pairs) >= FLOOR, (cls, len(pairs))
        for ge in (0, 1):
            sup, st = _oracle_suppressed(pairs, thr, plus_one, ge)
            assert (sup == EXPECT[cls][ge]).all(), (cls, ge)
            inter, uni, q = dc.iou_f32(st[:, 0], st[:, 1], plus_one)
            assert all(dc.iou_class(a, b, plus_one, thr) == cls for a, b in st)           # stacking moved nothing across a class border
            assert np.array_equal(dc.midpoint_iou_exceeds(inter, uni, thr, ge), sup), (cls, ge)
            naive = dc.naive_iou_exceeds(inter, uni, thr, ge)
            if (cls, ge) in (("above", 0), ("below", 1)):
                assert (naive != sup).all(), (cls, ge)
            fp32_naive_wrong += int((dc.naive_iou_exceeds(inter, uni, thr, ge, fp32_product=True) != sup).sum())
    assert fp32_naive_wrong > 0
    e = cases["exact"]   # some exact pairs have every side below 2^23: those survive the box coders' width + 1, so the decode paths see the class too
    assert ((e[:, :, 2] - e[:, :, 0] < 2 ** 23 - 1) & (e[:, :, 3] - e[:, :, 1] < 2 ** 23 - 1)).all(1).sum() >= 4


@pytest.mark.parametrize("plus_one", [0, 1])
def test_iou_windows_at_one_half(plus_one):
    """thr = 0.5f: the quotient is 0.5 only if it is exactly one half (iou_window_cases' docstring has the argument), so `above` and `below` are empty by
    arithmetic, not for want of searching; the other classes exist and behave as predicted."""
    thr = F32(0.5)
    cases = dc.iou_window_cases(thr, plus_one)
    assert len(cases["above"]) == 0 and len(cases["below"]) == 0
    for cls in ("exact", "pred", "succ"):
        assert len(cases[cls]) >= FLOOR, (cls, len(cases[cls]))
        for ge in (0, 1):
            sup, st = _oracle_suppressed(cases[cls], thr, plus_one, ge)
            assert (sup == EXPECT[cls][ge]).all(), (cls, ge)
            inter, uni, _ = dc.iou_f32(st[:, 0], st[:, 1], plus_one)
            assert np.array_equal(dc.midpoint_iou_exceeds(inter, uni, thr, ge), sup)


def test_degenerate_unions_take_the_not_positive_branch():
    """0/0, a negative union, inf and NaN: the forms the generator promises, and never a suppression, in the oracle and in the midpoint model."""
    forms = {}
    for name, a, b in dc.degenerate_union_pairs():
        inter, uni, q = dc.iou_f32(np.array(a, F32), np.array(b, F32), 0)
        forms[name] = (float(inter), float(uni), float(q))
        for thr in (0.7, 0.3, 0.5):
            for ge in (0, 1):
                keep = ora.nms(np.array([a, b], F32), np.array([1.0, 0.5], F32), thr, 0, ge)
                assert list(keep) == [0, 1], (name, thr, ge)
                assert not dc.midpoint_iou_exceeds(inter, uni, thr, ge)
    z, n, i, x = (forms[k] for k in ("zero_over_zero", "negative_union", "infinite_union", "nan_union"))
    assert z[0] == 0 and z[1] == 0 and np.isnan(z[2])
    assert n[0] == 0 and n[1] < 0 and n[2] == 0 and np.signbit(n[2])
    assert i[0] == 100 and i[1] == np.inf and i[2] == 0
    assert x[0] == np.inf and np.isnan(x[1]) and np.isnan(x[2])


@pytest.mark.parametrize("n,k", [(40, 13), (300, 100), (300, 128), (2000, 600), (9000, 200)])
def test_topk_key_sets_against_a_stable_sort(n, k):
    """ora.topk (qsort with the comparator value descending, index ascending; -0 == +0) against numpy's stable argsort of the negated keys, on every row;
    and the rows are what they claim to be."""
    rows = dict(dc.topk_key_sets(n, k, border=n // 2))
    for name, row in rows.items():
        s, i = ora.topk(row, k)
        rs, ri = dc.topk_reference(row, k)
        assert np.array_equal(i, ri), name
        assert np.array_equal(dc.bits(s), dc.bits(rs)), name
    cut = {name: dc.topk_reference(row, k)[0][-1] for name, row in rows.items()}
    for name in ("zero_cut", "all_zeros", "zero_cut_on_border"):
        sel, rest = dc.topk_reference(rows[name], k)[1], np.setdiff1d(np.arange(n), dc.topk_reference(rows[name], k)[1])
        assert cut[name] == 0
        for side in (sel, rest):                                      # zeros of both signs on both sides of the cut
            zs = rows[name][side][rows[name][side] == 0]
            assert np.signbit(zs).any() and (~np.signbit(zs)).any(), name
    sel = dc.topk_reference(rows["zero_cut_on_border"], k)[1]
    assert sel.max() == n // 2 - 1 and rows["zero_cut_on_border"][n // 2] == 0
    assert cut["neg_inf_cut"] == -np.inf and cut["subnormal_cut"] == dc.SUB_MIN and cut["neg_subnormal_cut"] == -dc.SUB_MIN
    # the order a bit-pattern sort gives (-0 below +0) differs from the contract on the simplest input
    s, i = ora.topk(np.array([-0.0, 0.0], F32), 1)
    assert list(i) == [0] and np.signbit(s[0])


def _ulp32(y):
    return np.spacing(np.abs(y).astype(F32)).astype(np.float64)


def test_detmath_against_float64_over_the_whole_domain():
    """The bounds of test_oracle_cpu.py::test_detmath_accuracy (there on linspace(-30, 30)) over detmath_inputs: every sign / exponent, subnormals, and the
    neighbourhood of every branch constant.  Measured on this sweep: exp 8.5e-8 (relative), sigmoid 8.9e-8, tanh 7.7e-8 (absolute); log2 exceeds half an ulp
    of its result by 3.6e-8 at most."""
    with np.errstate(all="ignore"):
        x = dc.detmath_inputs(dc.EXP).view(F32)
        x = x[np.isfinite(x)]
        x64 = x.astype(np.float64)
        m = (x64 >= -87.3) & (x64 <= 88.37)
        e = np.max(np.abs(ora.map_f32(x[m], dc.EXP).astype(np.float64) / np.exp(x64[m]) - 1))
        x = dc.detmath_inputs(dc.SIGMOID).view(F32)
        x = x[np.isfinite(x)]
        s = np.max(np.abs(ora.map_f32(x, dc.SIGMOID).astype(np.float64) - 1 / (1 + np.exp(-x.astype(np.float64)))))
        x = dc.detmath_inputs(dc.TANH).view(F32)
        x = x[np.isfinite(x)]
        t = np.max(np.abs(ora.map_f32(x, dc.TANH).astype(np.float64) - np.tanh(x.astype(np.float64))))
        x = dc.detmath_inputs(dc.LOG2).view(F32)
        assert ((x.view(U32) >> 23) >= 1).all() and ((x.view(U32) >> 23) <= 254).all()   # positive normal
        y = np.log2(x.astype(np.float64))
        excess = np.max(np.abs(ora.map_f32(x, dc.LOG2).astype(np.float64) - y) - 0.5 * _ulp32(y))
    print("detmath vs float64: exp rel %.3g, sigmoid abs %.3g, tanh abs %.3g, log2 excess over half an ulp %.3g" % (e, s, t, excess))
    assert e < 2.5e-7
    assert s < 1.5e-7
    assert t < 2e-7
    assert excess <= 1e-7   # measured 3.6e-8: the last step is one fmaf (half an ulp of the result), the rest is the polynomial's and ln's error


def test_detmath_special_values_by_bit_pattern():
    def f(fn, *v):
        return dc.bits(ora.map_f32(np.array(v, F32), fn))

    inf = np.inf
    assert list(f(dc.EXP, -inf)) == [0]
    assert list(f(dc.EXP, inf, 88.5)) == [0x7F3504A4, 0x7F3504A4]                         # the clamp's value ...
    assert F32(np.exp(np.float64(F32(dc.EXP_HI)))).view(U32) == 0x7F3504A4                 # ... which is the correctly rounded exp of the fp32 clamp
    assert list(f(dc.SIGMOID, -inf)) == [0x002D4151]                                       # 1 / (1 + the clamp's value): a subnormal
    assert list(f(dc.TANH, 0.0, -0.0)) == [0, 0]   # tanh(-0) is +0 here, not libm's -0: the last step is fmaf(t, x, x) with t = p * 0 = -0, and (-0)(-0) + (-0) = +0
    sub = np.array([1, 0x80000001], U32).view(F32)
    assert np.array_equal(dc.bits(ora.map_f32(sub, dc.TANH)), sub.view(U32))
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345], U32).view(F32)
    for fn in (dc.EXP, dc.SIGMOID, dc.TANH):
        assert np.isnan(ora.map_f32(nan, fn)).all(), fn


def test_detmath_inputs_hold_what_they_promise():
    for fn in (dc.EXP, dc.TANH):
        p = dc.detmath_inputs(fn)
        assert len(p) > 2_100_000 and len(np.unique(p)) == len(p)
        for special in (0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 1, 0x007FFFFF, 0x80000001):
            assert special in p[np.searchsorted(p, special): np.searchsorted(p, special) + 1], hex(special)
    pe = dc.detmath_inputs(dc.EXP)
    for c in (88.3762626647949, -87.3, (3 - 0.5) * np.log(2.0), (-100 - 0.5) * np.log(2.0)):
        b = dc.bits1(c)
        assert np.isin(np.arange(b - 4096, b + 4097), pe).all(), c
    pl = dc.detmath_inputs(dc.LOG2)
    b = dc.bits1(0.707106781186547524 * 2.0 ** -17)
    assert np.isin(np.arange(b - 4096, b + 4097), pl).all()


def test_threshold_logits_hit_the_threshold_exactly():
    thr, ncls = F32(0.05), 81
    rows = dc.threshold_logits(ora.softmax, thr, ncls, cls=ncls - 1)
    p = {k: ora.softmax(v[None])[0] for k, v in rows.items()}
    assert p["pred"][ncls - 1] == dc.f32_pred(thr) and p["on"][ncls - 1] == thr and p["succ"][ncls - 1] == dc.f32_succ(thr)
    for k in p:
        assert np.argmax(p[k][1:]) == ncls - 2                       # it is the row's best foreground class
    # the second_threshold construction: class 3 dominates, class 5 sits on the threshold
    rows = dc.threshold_logits(ora.softmax, thr, ncls, cls=5, also=(3, 2.0))
    for k, t in (("pred", dc.f32_pred(thr)), ("on", thr), ("succ", dc.f32_succ(thr))):
        q = ora.softmax(rows[k][None])[0]
        assert q[5] == t and np.argmax(q[1:]) == 2 and q[3] > 0.5


def test_threshold_logits_of_a_two_class_row():
    """Two classes: the foreground probability depends on x_fg - x_bg alone, and the oracle's softmax maps no fp32 difference onto 0.05f or its successor
    (checked here over the 4096 differences around the solution, for several background levels: the reachable set does not move).  The nearest reachable
    probabilities on either side are pred(0.05f) and 0.05f + 3 ulps."""
    thr = F32(0.05)
    rows = dc.threshold_logits(ora.softmax, thr, 2)
    assert "on" not in rows and "succ" not in rows
    pb, pa = ora.softmax(rows["below"][None])[0, 1], ora.softmax(rows["above"][None])[0, 1]
    assert pb == dc.f32_pred(thr) and dc.bits1(pa) - dc.bits1(thr) == 3
    for bg in (0.0, 0.125, 1.7, -3.3, 40.0):
        found, _, p = dc.find_logit(ora.softmax, np.array([bg, 0.0], F32), 1, [thr, dc.f32_succ(thr)])
        assert found[thr] is None and found[dc.f32_succ(thr)] is None
        assert p.min() < thr < p.max()


def test_knife_edge_masks():
    m = dc.knife_edge_masks((3, 28, 28), np.random.default_rng(0))
    assert m.dtype == F32 and set(np.unique(dc.bits(m))) == {0x3EFFFFFF, 0x3F000000, 0x3F000001}
