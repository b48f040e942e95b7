"""Independent restatement of COCO evaluation for the tests of isegmi.cocoeval.

It takes a different route from the product on purpose: every mask is decoded to a dense boolean plane, IoU is boolean algebra plus one float64
division, and matching / accumulate / summarize are plain Python loops written from the rule text of DESIGN.md section 10, not from the product's code.
Match arrays follow the product's documented convention: 1 + the partner's index inside its group (gts in annotation order, dets in descending
score order), 0 = unmatched."""
import numpy as np

from isegmi import coco


def dense(counts, h, w):
    flat = np.zeros(h * w, bool)
    pos, val = 0, False
    for c in counts:
        if val:
            flat[pos:pos + c] = True
        pos += c
        val = not val
    assert pos == h * w
    return flat.reshape((w, h)).T     # column-major


def seg_dense(seg, h, w):
    if isinstance(seg, dict):
        h, w = seg["size"]
        c = seg["counts"]
        return dense(coco.rle_from_string(c) if isinstance(c, str) else list(c), h, w)
    m = np.zeros((h, w), bool)
    for poly in seg:
        m |= dense(coco.rle_from_polygon(poly, h, w), h, w)
    return m


def mask_iou(d, g, crowd):
    inter = int(np.logical_and(d, g).sum())
    if inter == 0:
        return 0.0
    union = int(d.sum()) if crowd else int(np.logical_or(d, g).sum())
    return float(np.float64(inter) / np.float64(union))


def bbox_iou(d, g, crowd):
    """The stated operation order, float64."""
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    da = dw * dh; ga = gw * gh
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return float(i / u)


def tight_box(m):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def match_group(ious, det_area, gt_area, gt_crowd, gt_ignore, area_rng, iou_thrs):
    """ious [D][G] (dets in score order, gts in annotation order) -> dtm [A][T][D], dtig, gtm [A][T][G], gtig [A][G]."""
    D, G = len(det_area), len(gt_area)
    A, T = len(area_rng), len(iou_thrs)
    dtm = np.zeros((A, T, D), np.int32); dtig = np.zeros((A, T, D), np.uint8)
    gtm = np.zeros((A, T, G), np.int32); gtig = np.zeros((A, G), np.uint8)
    for a, (lo, hi) in enumerate(area_rng):
        ig = [bool(gt_ignore[g]) or bool(gt_crowd[g]) or gt_area[g] < lo or gt_area[g] > hi for g in range(G)]
        order = [g for g in range(G) if not ig[g]] + [g for g in range(G) if ig[g]]
        for g in range(G):
            gtig[a, g] = ig[g]
        for t, thr in enumerate(iou_thrs):
            for d in range(D):
                best = min(thr, 1 - 1e-10)
                m = -1
                for g in order:
                    if gtm[a, t, g] > 0 and not gt_crowd[g]:
                        continue
                    if m > -1 and not ig[m] and ig[g]:
                        break
                    if ious[d][g] < best:
                        continue
                    best = ious[d][g]
                    m = g
                if m == -1:
                    dtig[a, t, d] = det_area[d] < lo or det_area[d] > hi
                    continue
                dtig[a, t, d] = ig[m]
                dtm[a, t, d] = m + 1
                gtm[a, t, m] = d + 1
    return dtm, dtig, gtm, gtig


def evaluate(gt_dict, results, iou_type, img_ids, cat_ids, use_cats, max_dets, area_rng, iou_thrs):
    """-> {(category index, image index): group dict} like COCOeval.evalImgs, by dense masks."""
    imgs = {im["id"]: im for im in gt_dict["images"]}
    img_ids = sorted(set(img_ids)); cat_ids = sorted(set(cat_ids)) if use_cats else [-1]
    segm = iou_type == "segm"
    G, Dd = {}, {}
    for n, a in enumerate(gt_dict["annotations"]):
        im = imgs[a["image_id"]]
        m = seg_dense(a["segmentation"], im["height"], im["width"]) if a.get("segmentation") is not None else None
        area = float(a["area"]) if "area" in a else float(m.sum())
        box = [float(v) for v in a["bbox"]] if "bbox" in a else tight_box(m)
        key = (a["category_id"] if use_cats else -1, a["image_id"])
        G.setdefault(key, []).append({"mask": m, "area": area, "box": box, "crowd": int(a.get("iscrowd", 0)), "ignore": int(a.get("ignore", 0))})
    for n, r in enumerate(results):
        im = imgs[r["image_id"]]
        m = seg_dense(r["segmentation"], im["height"], im["width"]) if r.get("segmentation") is not None else None
        if segm:
            area, box = float(m.sum()), None
        else:
            box = [float(v) for v in r["bbox"]] if r.get("bbox") is not None else tight_box(m)
            area = box[2] * box[3]
        key = (r["category_id"] if use_cats else -1, r["image_id"])
        Dd.setdefault(key, []).append({"mask": m, "area": area, "box": box, "score": float(r["score"]), "n": n})
    out = {}
    for k, c in enumerate(cat_ids):
        for i, iid in enumerate(img_ids):
            gts = G.get((c, iid), []); dts = Dd.get((c, iid), [])
            if not gts and not dts:
                continue
            dts = sorted(dts, key=lambda d: -d["score"])[:max_dets[-1]]     # Python's sort is stable
            ious = [[(mask_iou(d["mask"], g["mask"], g["crowd"]) if segm else bbox_iou(d["box"], g["box"], g["crowd"])) for g in gts] for d in dts]
            dtm, dtig, gtm, gtig = match_group(ious, [d["area"] for d in dts], [g["area"] for g in gts], [g["crowd"] for g in gts],
                                               [g["ignore"] for g in gts], area_rng, iou_thrs)
            out[(k, i)] = {"dtScores": np.array([d["score"] for d in dts], np.float64), "dtMatches": dtm, "dtIgnore": dtig, "gtMatches": gtm,
                           "gtIgnore": gtig, "ious": np.array(ious, np.float64).reshape(len(dts), len(gts))}
    return out


def accumulate(eval_imgs, n_cats, max_dets, n_area, iou_thrs, rec_thrs):
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), n_cats, n_area, len(max_dets)
    precision = -np.ones((T, R, K, A, M)); recall = -np.ones((T, K, A, M)); scores = -np.ones((T, R, K, A, M))
    eps = np.spacing(1)
    for k in range(K):
        E = [eval_imgs[key] for key in sorted(eval_imgs) if key[0] == k]
        if not E:
            continue
        for a in range(A):
            npig = sum(int(v == 0) for e in E for v in e["gtIgnore"][a])
            if npig == 0:
                continue
            for m, md in enumerate(max_dets):
                for t in range(T):
                    rows = []   # (score, matched, ignored) in concatenation order
                    for e in E:
                        for d in range(min(md, len(e["dtScores"]))):
                            rows.append((float(e["dtScores"][d]), int(e["dtMatches"][a][t][d]) != 0, int(e["dtIgnore"][a][t][d]) != 0))
                    rows.sort(key=lambda r: -r[0])   # stable
                    tp = fp = 0
                    rc, pr = [], []
                    for s, matched, ign in rows:
                        if not ign:
                            tp += matched; fp += not matched
                        rc.append(np.float64(tp) / npig)
                        pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + eps))
                    recall[t, k, a, m] = rc[-1] if rows else 0
                    for j in range(len(pr) - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    for r, thr in enumerate(rec_thrs):
                        j = 0
                        while j < len(rc) and rc[j] < thr:
                            j += 1
                        precision[t, r, k, a, m] = pr[j] if j < len(rc) else 0.0
                        scores[t, r, k, a, m] = rows[j][0] if j < len(rc) else 0.0
    return precision, recall, scores


def summarize(precision, recall, iou_thrs, max_dets):
    def mean(x):
        v = [float(s) for s in x.ravel() if s > -1]
        return -1.0 if not v else float(np.mean(np.array(v)))
    t50 = int(np.argmin(np.abs(np.asarray(iou_thrs) - 0.5))); t75 = int(np.argmin(np.abs(np.asarray(iou_thrs) - 0.75)))
    M = len(max_dets) - 1
    return np.array([mean(precision[:, :, :, 0, M]), mean(precision[t50, :, :, 0, M]), mean(precision[t75, :, :, 0, M]),
                     mean(precision[:, :, :, 1, M]), mean(precision[:, :, :, 2, M]), mean(precision[:, :, :, 3, M]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, min(1, M)]), mean(recall[:, :, 0, M]),
                     mean(recall[:, :, 1, M]), mean(recall[:, :, 2, M]), mean(recall[:, :, 3, M])])
