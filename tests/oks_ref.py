"""Independent restatement of COCO keypoint evaluation for the tests of isegmi.cocoeval under "keypoints" (DESIGN.md section 10).

It takes a different route from the product on purpose: the object keypoint similarity (OKS) of a pair is a plain Python loop over the keypoints
with numpy float64 scalars, np.exp on one scalar at a time and the terms added in keypoint-index order; grouping and the ten numbers are loops
written from the rule text of DESIGN.md section 10.  Matching and accumulate are cocoeval_ref's loops.  oks_decimal is the arbiter for the last
bits: the same exp arguments, then exp, the sum and the division in 50-digit decimal arithmetic."""
import decimal

import numpy as np

import cocoeval_ref as ref

F = np.float64
SIGMAS = list(np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0)   # as upstream writes them
KPT_AREA_RNG = [[0.0, 1e10], [1024.0, 9216.0], [9216.0, 1e10]]


def variances(sigmas):
    """(sigmas * 2) ** 2 by numpy, exactly as upstream writes it."""
    return (np.asarray(sigmas, np.float64) * 2) ** 2


def exp_args(dk, gk, gbox, garea, var, variant=None):
    """-> (the counted keypoint indices, their e as float64 scalars).  dk, gk: K * 3 numbers (x, y, v).
    variant (for the fixture's self-check only): "det_v" also wants the DETECTION's v > 0, "no_eps" drops spacing(1) from the denominator."""
    K = len(var)
    vis = [k for k in range(K) if gk[3 * k + 2] > 0]
    den = F(garea) + (F(0) if variant == "no_eps" else np.spacing(F(1)))
    idx, es = [], []
    with np.errstate(all="ignore"):
        if vis:
            for k in vis:
                if variant == "det_v" and not dk[3 * k + 2] > 0:
                    continue
                dx = F(dk[3 * k]) - F(gk[3 * k]); dy = F(dk[3 * k + 1]) - F(gk[3 * k + 1])
                idx.append(k); es.append((dx * dx + dy * dy) / F(var[k]) / den / F(2))
        else:
            bx, by, bw, bh = (F(v) for v in gbox)
            x0 = bx - bw; x1 = bx + bw * F(2); y0 = by - bh; y1 = by + bh * F(2)
            for k in range(K):
                xd, yd = F(dk[3 * k]), F(dk[3 * k + 1])
                dx = max(F(0), x0 - xd) + max(F(0), xd - x1); dy = max(F(0), y0 - yd) + max(F(0), yd - y1)
                idx.append(k); es.append((dx * dx + dy * dy) / F(var[k]) / den / F(2))
    return idx, es


def oks_pair(dk, gk, gbox, garea, var, variant=None):
    """OKS of one (detection, ground truth) pair, the terms added in keypoint-index order.  variant "div_K" divides by K whatever k1 is."""
    K = len(var)
    k1 = sum(1 for k in range(K) if gk[3 * k + 2] > 0)
    _, es = exp_args(dk, gk, gbox, garea, var, variant)
    s = F(0)
    with np.errstate(all="ignore"):
        for e in es:
            s = s + np.exp(-e)
        n = K if (variant == "div_K" or k1 == 0) else k1
        return float(s / F(n))


def oks_np_sum(dk, gk, gbox, garea, var):
    """The same terms added by np.sum (upstream's order) -- only to show how far the two orders can differ."""
    K = len(var)
    k1 = sum(1 for k in range(K) if gk[3 * k + 2] > 0)
    _, es = exp_args(dk, gk, gbox, garea, var)
    return float(np.sum(np.exp(-np.array(es, np.float64))) / F(k1 if k1 else K))


def oks_decimal(dk, gk, gbox, garea, var):
    """The arbiter: the float64 exp arguments of exp_args, then exp, sum and division in 50-digit decimal arithmetic -> decimal.Decimal."""
    K = len(var)
    k1 = sum(1 for k in range(K) if gk[3 * k + 2] > 0)
    _, es = exp_args(dk, gk, gbox, garea, var)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        ctx.Emin = -999999; ctx.traps[decimal.Underflow] = False; ctx.traps[decimal.Inexact] = False
        s = decimal.Decimal(0)
        for e in es:
            fe = float(e)
            s += decimal.Decimal(0) if fe > 1e5 else (-decimal.Decimal(fe)).exp()      # exp(-1e5) < 1e-43000: nothing next to a sum >= 0
        return s / decimal.Decimal(k1 if k1 else K)


def extent(kp):
    """loadRes' keypoint branch: area and xywh box of the extents of x and y."""
    xs, ys = [float(v) for v in kp[0::3]], [float(v) for v in kp[1::3]]
    x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
    return (x1 - x0) * (y1 - y0), [x0, y0, x1 - x0, y1 - y0]


def evaluate(gt_dict, results, sigmas, max_det=20, area_rng=KPT_AREA_RNG, iou_thrs=None, variant=None):
    """-> {(category index, image index): group dict} like COCOeval.evalImgs under "keypoints"."""
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else iou_thrs
    var = variances(sigmas)
    img_ids = sorted(im["id"] for im in gt_dict["images"])
    cat_ids = sorted(c["id"] for c in gt_dict["categories"])
    G, D = {}, {}
    for a in gt_dict["annotations"]:
        nk = a["num_keypoints"] if "num_keypoints" in a else sum(1 for v in a["keypoints"][2::3] if v > 0)
        G.setdefault((a["category_id"], a["image_id"]), []).append(
            {"kp": a["keypoints"], "box": a["bbox"], "area": float(a["area"]), "crowd": int(a.get("iscrowd", 0)),
             "ignore": int(bool(a.get("ignore", 0)) or nk == 0)})
    for r in results:
        D.setdefault((r["category_id"], r["image_id"]), []).append({"kp": r["keypoints"], "area": extent(r["keypoints"])[0], "score": float(r["score"])})
    out = {}
    for k, c in enumerate(cat_ids):
        for i, iid in enumerate(img_ids):
            gts, dts = G.get((c, iid), []), D.get((c, iid), [])
            if not gts and not dts:
                continue
            dts = sorted(dts, key=lambda d: -d["score"])[:max_det]     # Python's sort is stable
            oks = [[oks_pair(d["kp"], g["kp"], g["box"], g["area"], var, variant) for g in gts] for d in dts]
            dtm, dtig, gtm, gtig = ref.match_group(oks, [d["area"] for d in dts], [g["area"] for g in gts], [g["crowd"] for g in gts],
                                                   [g["ignore"] for g in gts], area_rng, iou_thrs)
            out[(k, i)] = {"dtScores": np.array([d["score"] for d in dts], np.float64), "dtMatches": dtm, "dtIgnore": dtig, "gtMatches": gtm,
                           "gtIgnore": gtig, "ious": np.array(oks, np.float64).reshape(len(dts), len(gts))}
    return out


def summarize(precision, recall, iou_thrs):
    """The ten keypoint numbers: AP, AP@.5, AP@.75, AP medium, AP large, then the same five of AR; area ranges (all, medium, large), one maxDets."""
    def mean(x):
        v = [float(s) for s in x.ravel() if s > -1]
        return -1.0 if not v else float(np.mean(np.array(v)))
    t50 = int(np.argmin(np.abs(np.asarray(iou_thrs) - 0.5))); t75 = int(np.argmin(np.abs(np.asarray(iou_thrs) - 0.75)))
    return np.array([mean(precision[:, :, :, 0, 0]), mean(precision[t50, :, :, 0, 0]), mean(precision[t75, :, :, 0, 0]),
                     mean(precision[:, :, :, 1, 0]), mean(precision[:, :, :, 2, 0]),
                     mean(recall[:, :, 0, 0]), mean(recall[t50, :, 0, 0]), mean(recall[t75, :, 0, 0]), mean(recall[:, :, 1, 0]), mean(recall[:, :, 2, 0])])


def lines(stats, max_det=20):
    """The ten lines of upstream's keypoint summary for ten numbers."""
    rows = [("0.50:0.95", "all"), ("0.50", "all"), ("0.75", "all"), ("0.50:0.95", "medium"), ("0.50:0.95", "large")]
    out = []
    for j, s in enumerate(stats):
        title, kind = ("Average Precision", "(AP)") if j < 5 else ("Average Recall", "(AR)")
        iou, area = rows[j % 5]
        out.append(" %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f" % (title, kind, iou, area, max_det, s))
    return out
