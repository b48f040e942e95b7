"""Inputs that sit ON the detection tail's discrete decisions (TEST INFRASTRUCTURE ONLY, numpy only), shared by tests/test_decision_edges_gpu.py (HIP kernel
against the CPU oracle, bit for bit) and tests/test_decision_cases_cpu.py (the proof that these inputs discriminate: the oracle gives the verdict each class
predicts, a naive restatement of the decision gives the opposite one, and the oracle's own math stays inside its bounds at every input used here).

  iou_window_cases     box pairs whose fp32 IoU quotient is thr, or one ulp from it, classified by the exact rational inter / uni
  degenerate_union_pairs   0/0, negative, infinite and NaN unions
  topk_key_sets        rows of special float keys (zeros of both signs, subnormals, +-FLT_MAX, +-inf) with the k-th key a zero, -inf, a subnormal
  detmath_inputs       bit patterns: a sweep over every sign / exponent, and +-4096 patterns around every branch constant of the four functions
  find_logit / threshold_logits   softmax rows whose foreground probability is exactly pred(thr), thr, succ(thr)
  knife_edge_masks     mask probabilities drawn from {pred(0.5), 0.5, succ(0.5)}
Everything is deterministic (seeded)."""
from fractions import Fraction

import numpy as np

F32 = np.float32
U32 = np.uint32
INF = F32(np.inf)


def f32_succ(x):
    return np.nextafter(F32(x), INF)


def f32_pred(x):
    return np.nextafter(F32(x), -INF)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def bits1(x):
    """the bit pattern of one float32 as a Python int"""
    return int(np.array([x], F32).view(U32)[0])


# ------------------------------------------------------------------------------------------------------------------ IoU windows
IOU_CLASSES = ("above", "below", "pred", "succ", "exact")   # on-from-above, on-from-below, one ulp either side, the rational equals thr


def iou_f32(a, b, one):
    """inter, uni, q = RN(inter / uni) of boxes a, b [..., 4] in np.float32 arithmetic, in the oracle's operation order (ora_ops.c iou_plus; with one = 0
    also Yolact's jaccard1, whose only difference is the absent `+ 0`)."""
    a = np.asarray(a, F32); b = np.asarray(b, F32); one = F32(one)
    with np.errstate(all="ignore"):
        aa = (a[..., 2] - a[..., 0] + one) * (a[..., 3] - a[..., 1] + one)
        ab = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
        xx1 = np.where(a[..., 0] > b[..., 0], a[..., 0], b[..., 0]); yy1 = np.where(a[..., 1] > b[..., 1], a[..., 1], b[..., 1])
        xx2 = np.where(a[..., 2] < b[..., 2], a[..., 2], b[..., 2]); yy2 = np.where(a[..., 3] < b[..., 3], a[..., 3], b[..., 3])
        w = xx2 - xx1 + one; h = yy2 - yy1 + one
        w = np.where(w > 0, w, F32(0)); h = np.where(h > 0, h, F32(0))
        inter = w * h
        uni = aa + ab - inter
        q = inter / uni
    assert inter.dtype == F32 and uni.dtype == F32 and q.dtype == F32
    return inter, uni, q


def iou_class(a, b, one, thr):
    """The class of one pair: by the fp32 quotient and, where that equals thr, by the EXACT rational inter / uni of the fp32 inter and uni (what both the
    oracle's division and the device's midpoint comparison start from).  None: the pair is in no class."""
    inter, uni, q = iou_f32(a, b, one)
    thr = F32(thr)
    if not (np.isfinite(inter) and np.isfinite(uni) and uni > 0):
        return None
    if q == f32_pred(thr):
        return "pred"
    if q == f32_succ(thr):
        return "succ"
    if q != thr:
        return None
    x, t = Fraction(float(inter)) / Fraction(float(uni)), Fraction(float(thr))
    return "exact" if x == t else ("above" if x > t else "below")


def _strip_pair(U, I, one, H=1, xb=0, Hb=None, yb=0):
    """A = U wide and H high at the origin, B = I wide and Hb (default H) high at offset (xb, yb) inside A; `one` = 1: legacy inclusive corners."""
    Hb = H if Hb is None else Hb
    return np.array([[0, 0, U - one, H - one], [xb, yb, xb + I - one, yb + Hb - one]], np.float64)


def _exact_geometries(t, max_h):
    """(W, Ha, Wb, Hb) with Wb Hb / (W Ha) == t exactly, B fitting into A, every side below 2^23 (so that the box coders' width + 1 stays an fp32 number)
    and Ha <= max_h: for t = num / 2^24 that takes a divisor b of num (Wb = num / b, Hb = b h) and W Ha = 2^24 h."""
    out = []
    for b in (d for d in range(1, max_h + 1) if t.numerator % d == 0):
        Wb = t.numerator // b
        if Wb >= 2 ** 23:
            continue
        for h in range(1, max_h // b + 1):
            Hb = b * h
            Ha = np.arange(Hb, max_h + 1, dtype=np.int64)
            Ha = Ha[(t.denominator * h) % Ha == 0]
            W = t.denominator * h // Ha
            ok = (W >= Wb) & (W < 2 ** 23)
            out += [(int(w), int(a), Wb, Hb) for w, a in zip(W[ok], Ha[ok])]
    return out


def iou_window_cases(thr, plus_one, per_class=48, seed=0):
    """{class: float32 [n, 2, 4]} pairs (A, B), B inside A, at y = 0 (stack_pairs moves them apart).  Long thin strips of integer width U < 2^23 (2^24 for
    thr = 0.5) and I ~ thr * U, so inter = I and uni = U exactly; the classes come from where RN(I / U) falls.  The `exact` class of a thr whose
    denominator is 2^24 (0.7f, 0.3f) needs a union that is a multiple of 2^24.  Half of those pairs are 2-D with every side below 2^23
    (_exact_geometries: e.g. A = 8192 x 2048, B = 7793 x 1507 for 0.7f = 11 * 137 * 7793 / 2^24), which every box coder reproduces; the other half has A 2^24 wide and
    H <= 64 high with B thr * 2^24 wide.  In both families only the geometries for which the fp32 `aa + ab - inter` rounds back to the exact union
    qualify.  Every returned pair is classified by iou_class() on its final float32 coordinates.

    thr = 0.5f has no `above` / `below` pair at ANY size: q = RN(inter / uni) = 0.5 with inter / uni != 0.5 needs |2 inter - uni| < uni * 2^-24, but for
    fp32 inter in [2^(e-1), 2^e) and uni in [2^e, 2^(e+1)) both 2 inter and uni are multiples of 2^(e-23) > uni * 2^-24, so 2 inter - uni is 0 or too
    large.  (inter and uni are fp32 results, whatever the boxes.)  Those two lists come back empty for 0.5."""
    thr = F32(thr); one = 1 if plus_one else 0
    t = Fraction(float(thr))
    rng = np.random.default_rng(seed * 7919 + bits1(thr) % 100003 + one)
    out = {c: [] for c in IOU_CLASSES}

    def offer(pair, cap=per_class):
        p32 = pair.astype(F32)
        assert np.array_equal(p32.astype(np.float64), pair)          # coordinates exactly representable
        c = iou_class(p32[0], p32[1], one, thr)
        if c is not None and len(out[c]) < cap:
            out[c].append(p32)

    hi = 2 ** 24 if t.denominator <= 2 ** 23 else 2 ** 23
    U = rng.integers(2 ** 20, hi, 200000)
    I0 = np.rint(float(thr) * U).astype(np.int64)
    for dI in (0, -1, 1):
        I = I0 + dI
        q = I.astype(F32) / U.astype(F32)
        sgn = np.sign(I * t.denominator - t.numerator * U)            # sign of I / U - thr, exact in int64 (< 2^50)
        for cls, m in (("pred", q == f32_pred(thr)), ("succ", q == f32_succ(thr)), ("above", (q == thr) & (sgn > 0)), ("below", (q == thr) & (sgn < 0)),
                       ("exact", (q == thr) & (sgn == 0))):
            for j in np.nonzero(m)[0][: per_class]:
                if len(out[cls]) < per_class:
                    offer(_strip_pair(int(U[j]), int(I[j]), one))
    if t.denominator > 2 ** 23:                                       # exact: uni must be a multiple of the denominator
        W, Wb = t.denominator, t.numerator
        assert W == 2 ** 24
        geos = _exact_geometries(t, PAIR_PITCH - 8)
        for g in rng.permutation(len(geos))[:600]:                    # the 2-D family first: up to half of the class
            Wa, Ha, Wb2, Hb = geos[g]
            if len(out["exact"]) >= per_class // 2:
                break
            for rep in range(4):                                      # (the offsets move no area: a geometry qualifies with all of them or with none)
                offer(_strip_pair(Wa, Wb2, one, H=Ha, xb=int(rng.integers(0, Wa - Wb2 + 1)), Hb=Hb, yb=int(rng.integers(0, Ha - Hb + 1))), cap=per_class // 2)
        for xb in rng.integers(0, min(W - Wb, 2 ** 21), 12):
            for H in range(1, 65):
                offer(_strip_pair(W, Wb, one, H=H, xb=int(xb)))
    return {c: (np.stack(v) if v else np.zeros((0, 2, 4), F32)) for c, v in out.items()}


PAIR_PITCH = 4096   # > the tallest pair (4088): pairs at different slots never overlap, and every y stays a small integer (exact in fp32)


def stack_pairs(pairs, first_slot=0):
    """pairs [n, 2, 4] at y = 0 -> the same pairs at y = slot * PAIR_PITCH, so that only A_i and B_i overlap."""
    p = np.array(pairs, F32, copy=True)
    y = (np.arange(len(p), dtype=F32) + F32(first_slot)) * F32(PAIR_PITCH)
    p[:, :, 1] += y[:, None]; p[:, :, 3] += y[:, None]
    return p


def degenerate_union_pairs():
    """[(name, A, B)] for plain areas (plus_one = 0): unions that are 0, negative, +inf and NaN.  In every one of them `iou > thr` and `iou >= thr` are both
    false for thr > 0 (the quotient is NaN, -0, 0, NaN), so B is kept."""
    big = 2e19   # (2e19)^2 = 4e38 > FLT_MAX
    return [
        ("zero_over_zero", [5, 5, 5, 5], [5, 5, 5, 5]),                                   # areas 0, inter 0: 0 / 0 = NaN
        ("negative_union", [10, 0, 0, 10], [10, 0, 0, 10]),                               # x corners reversed: areas -100, inter 0, union -200: -0
        ("infinite_union", [0, 0, big, big], [-big, -big, 10, 10]),                       # areas +inf, inter 100, union +inf: 0
        ("nan_union", [0, 0, big, big], [0, 0, big, big]),                                # inter +inf, union inf - inf = NaN
    ]


def naive_iou_exceeds(inter, uni, thr, ge, fp32_product=False):
    """The predicate a division-free NMS must NOT use: inter > thr * uni.  Default: the product in fp64, where it is exact (24 x 24 bits) -- iou_exceeds()
    with thr in the place of its midpoint, i.e. the comparison of the REAL quotient with thr.  fp32_product: the product rounded to fp32 first (a different
    wrong answer: it rounds thr * uni onto inter in both `on` classes and errs one ulp further out instead)."""
    inter = np.asarray(inter, F32); uni = np.asarray(uni, F32)
    if fp32_product:
        lhs, rhs = inter, F32(thr) * uni
    else:
        lhs, rhs = inter.astype(np.float64), np.float64(F32(thr)) * uni.astype(np.float64)
    return (lhs >= rhs) if ge else (lhs > rhs)


def midpoint_iou_exceeds(inter, uni, thr, ge):
    """numpy restatement of csrc/detbox.h make_iou_thr / iou_exceeds: the real quotient against the midpoint between thr and its fp32 neighbour, in fp64
    (exact: 24-bit inter and uni, 25-bit midpoint), ties to the even mantissa; a union that is not > 0 never exceeds."""
    thr = F32(thr)
    b = bits1(thr)
    if ge:
        lo = np.array(b - 1, U32).view(F32)
        m, tie = 0.5 * (np.float64(lo) + np.float64(thr)), (b & 1) == 0
    else:
        hi = np.array(b + 1, U32).view(F32)
        m, tie = 0.5 * (np.float64(thr) + np.float64(hi)), ((b + 1) & 1) == 0
    inter = np.asarray(inter, F32); uni = np.asarray(uni, F32)
    with np.errstate(all="ignore"):
        lhs, rhs = inter.astype(np.float64), m * uni.astype(np.float64)
        return (uni > 0) & ((lhs > rhs) | ((lhs == rhs) & tie))


# ------------------------------------------------------------------------------------------------------------------ top-k keys
def _u2f(u):
    return np.array(u, U32).view(F32)


SUB_MIN, SUB_MAX, NORM_MIN, FLT_MAX = _u2f(1), _u2f(0x007FFFFF), _u2f(0x00800000), _u2f(0x7F7FFFFF)
POSITIVES = np.array([SUB_MIN, SUB_MAX, NORM_MIN, FLT_MAX, np.inf, 0.5, 1.0, 3.25, 1e-30, 7e20], F32)


def _scatter(rng, n, groups):
    """groups: [(values, count)] -> a row of n keys with every group's values at random positions (so the groups interleave in index order)."""
    row = np.concatenate([np.resize(np.asarray(v, F32), c) for v, c in groups if c > 0])
    assert row.size == n, (row.size, n)
    return row[rng.permutation(n)]


def _alternate_zeros(row, ends_only=False):
    """the zeros of `row` get alternating signs in index order, -0 first (ends_only: just the first two and the last two): both signs on both sides of a cut"""
    z = np.nonzero(row == 0)[0]
    if ends_only:
        z = np.concatenate([z[:2], z[-2:]])
    row[z] = np.resize(np.array([-0.0, 0.0], F32), z.size)
    return row


def topk_key_sets(n, k, seed=0, border=None):
    """[(name, float32 row [n])]: the k-th key in (value descending, index ascending) order is a zero with zeros of both signs on both sides of the cut; all
    keys are zeros of mixed sign; the k-th key is -inf; the k-th key is a subnormal with equal subnormals on both sides of the cut.  No NaN.
    border (an index): one more row whose zero-valued cut falls exactly there -- the last selected zero is key border - 1 (the two-level kernel's slice
    border).  Needs 4 <= k < n - 8."""
    assert 4 <= k < n - 8
    rng = np.random.default_rng(seed * 1000003 + n * 31 + k)
    zeros = np.array([0.0, -0.0], F32)
    neg = -POSITIVES
    a = k - 3                         # keys strictly above the cut value; the cut takes 3 of the equal ones
    eq = min(n - a, max(8, (n - a) // 2))
    rows = [
        ("zero_cut", _alternate_zeros(_scatter(rng, n, [(rng.choice(POSITIVES, a), a), ([0.0], eq), (rng.choice(neg, n - a - eq), n - a - eq)]))),
        ("all_zeros", _alternate_zeros(rng.choice(zeros, n).astype(F32), ends_only=True)),
        ("neg_inf_cut", _scatter(rng, n, [(rng.choice(np.concatenate([POSITIVES, zeros, neg[neg > -np.inf]]), a), a), ([-np.inf], n - a)])),
        ("subnormal_cut", _scatter(rng, n, [(rng.choice(POSITIVES[1:], a), a), ([SUB_MIN], eq),
                                           (rng.choice(np.concatenate([zeros, neg]), n - a - eq), n - a - eq)])),
        ("neg_subnormal_cut", _scatter(rng, n, [(rng.choice(np.concatenate([POSITIVES, zeros]), a), a), ([-SUB_MIN], eq),
                                               (rng.choice(neg[1:], n - a - eq), n - a - eq)])),
    ]
    if border is not None:
        assert a + 6 <= border <= n - 6
        row = rng.choice(neg, n).astype(F32)
        row[rng.choice(border - 6, a, replace=False)] = rng.choice(POSITIVES, a)
        row[border - 6: border + 6] = np.resize(np.array([-0.0, 0.0, 0.0, -0.0], F32), 12)   # the cut takes border-3 .. border-1
        row[border - 6: border - 3] = rng.choice(neg, 3)
        rows.append(("zero_cut_on_border", row))
    for name, r in rows:
        assert r.dtype == F32 and r.shape == (n,) and not np.isnan(r).any(), name
    return rows


def topk_reference(row, k):
    """(value descending with zeros equal, index ascending): numpy's STABLE argsort of the negated keys -- the independent reference for ora.topk."""
    row = np.asarray(row, F32)
    idx = np.argsort(-row, kind="stable")[: min(k, row.size)]
    return row[idx], idx.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ detmath
EXP, SIGMOID, TANH, LOG2 = 0, 1, 2, 3
EXP_HI, EXP_LO = 88.3762626647949, -87.3


def _windows(centres, half=4096):
    c = np.ascontiguousarray(centres, F32).view(U32).astype(np.int64)
    w = c[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    w = w[(w >= 0)]
    return w.reshape(-1)


def detmath_inputs(fn):
    """uint32 bit patterns for ora / isegmi map_f32(fn): every sign / exponent (512) x {every 2^11-th mantissa, the 64 lowest, the 64 highest} -- that holds
    +-0, +-inf, quiet and signalling-pattern NaNs of both signs and 2 x 4224 subnormals -- plus +-4096 consecutive patterns around every branch constant:
    exp (and sigmoid, which is exp(-x)): the clamp 88.376..., the cut -87.3, +-0 and the 255 steps of floorf(x log2e + 0.5) at (k - 0.5) ln 2, both signs;
    tanh: +-0.625, +-44, +-0 and half of exp's points (tanh calls exp(2|x|));  log2: 0.70710678 * 2^e and 2^e for every normal exponent.
    log2 gets positive normal inputs only (its stated domain)."""
    mant = np.unique(np.concatenate([np.arange(0, 1 << 23, 1 << 11), np.arange(64), (1 << 23) - 1 - np.arange(64)])).astype(np.int64)
    se = np.arange(512, dtype=np.int64) << 23
    pats = [(se[:, None] | mant[None, :]).reshape(-1)]
    steps = ((np.arange(-126, 129) - 0.5) * np.log(2.0)).astype(F32)
    if fn in (EXP, SIGMOID):
        c = np.concatenate([[EXP_HI, EXP_LO, 0.0], steps]).astype(F32)
        pats.append(_windows(np.concatenate([c, -c])))
    elif fn == TANH:
        c = np.concatenate([[0.625, 44.0, 0.0, EXP_HI / 2], steps[steps > 0] / 2]).astype(F32)
        pats.append(_windows(np.concatenate([c, -c])))
    else:
        e = np.arange(-126, 128).astype(np.float64)
        pats.append(_windows(np.concatenate([np.float64(F32(0.707106781186547524)) * 2.0 ** e, 2.0 ** e]).astype(F32)))
    p = np.unique(np.concatenate(pats))
    p = p[(p >= 0) & (p <= 0xFFFFFFFF)]
    if fn == LOG2:
        p = p[(p >= 0x00800000) & (p < 0x7F800000)]
    return p.astype(U32)


# ------------------------------------------------------------------------------------------------------------------ thresholds
def find_logit(softmax, template, slot, targets, span=2048):
    """Rows equal to `template` except for logit `slot`, whose softmax probability (by `softmax`, the oracle's: rows [r, C] -> [r, C]) is exactly each of
    `targets`: 2 * span consecutive bit patterns of that logit around the float64 solution are tried.  ({target: row or None}, the tried rows, their
    probabilities of class `slot`)."""
    template = np.asarray(template, F32)
    others = np.delete(template.astype(np.float64), slot)
    found = {F32(t): None for t in targets}
    t0 = float(np.median([float(t) for t in targets]))
    x0 = F32(np.log(t0 / (1.0 - t0) * np.exp(others - others.max()).sum()) + others.max())
    cand = (bits1(x0) + np.arange(-span, span, dtype=np.int64)).astype(U32).view(F32)
    rows = np.repeat(template[None], cand.size, 0)
    rows[:, slot] = cand
    p = softmax(rows)[:, slot]
    for t in found:
        hit = np.nonzero(p == t)[0]
        if hit.size:
            found[t] = rows[hit[0]].copy()
    return found, rows, p


def threshold_logits(softmax, thr, ncls, cls=1, also=None, seed=0):
    """{"pred" | "on" | "succ": float32 row [ncls]} whose probability of class `cls` is exactly pred(thr), thr, succ(thr) under the oracle's softmax, the
    background (class 0) being the row's largest logit.  One logit moves the probability ~3 ulps per ulp of its own, so a single search reaches about one
    target in three; a third class (the `tuner`, probability below thr / 2) shifts the sum by fractions of an ulp, and it walks until every target is hit.
    ncls = 2 has no third class: the probability is a function of the ONE fp32 number x_fg - x_bg, the reachable values around 0.05f are fixed
    (..., thr - 1 ulp, thr + 3 ulps, ...), and thr and succ(thr) are not among them.  The result then holds what exists, and always "below" / "above": the
    reachable probabilities nearest to thr on either side (below: the largest p <= thr).
    also = (class, offset above the background): one dominant foreground class, so that the row passes a best-class pre-filter whatever `cls` scores."""
    thr = F32(thr)
    want = {"pred": f32_pred(thr), "on": thr, "succ": f32_succ(thr)}
    rng = np.random.default_rng(seed + ncls)
    tuner = None if ncls == 2 else next(c for c in range(1, ncls) if c != cls and (also is None or c != also[0]))
    got = {}
    for step in range(1 if tuner is None else 256):
        tmpl = (-20.0 - rng.uniform(0, 1, ncls)).astype(F32)
        tmpl[0] = 0.0
        if also is not None:
            tmpl[also[0]] = F32(also[1])
        if tuner is not None:
            tmpl[tuner] = F32(-4.0) - F32(step) * F32(1.0 / 64)
        found, rows, p = find_logit(softmax, tmpl, cls, list(want.values()))
        if step == 0:
            got["below"] = rows[np.nonzero(p <= thr)[0][np.argmax(p[p <= thr])]].copy()
            got["above"] = rows[np.nonzero(p > thr)[0][np.argmin(p[p > thr])]].copy()
        for name, row in zip(want, found.values()):
            if row is not None and name not in got:
                got[name] = row
        if all(n in got for n in want):
            break
    assert tuner is None or all(n in got for n in want), sorted(set(want) - set(got))
    return got


def knife_edge_masks(shape, rng):
    """fp32 mask probabilities drawn from {pred(0.5), 0.5, succ(0.5)}: every bilinear blend of them is within an ulp or two of the 0.5 threshold."""
    return rng.choice(np.array([f32_pred(0.5), 0.5, f32_succ(0.5)], F32), shape).astype(F32)
