"""Seeded synthetic COCO annotation sets and result lists for the tests of isegmi.cocoeval.

Covers: gts as polygons (one or several parts), uncompressed and compressed RLEs; crowd regions; dets as perturbed gts plus false positives; tied
scores; dets identical to a gt (IoU exactly 1.0); empty masks; images with no gt or no det; a category with only crowd gts; a category with no gt;
gt id 0; small rectangle pairs whose IoU sits exactly on a threshold (2x3 in 2x4 = 0.75, 2x2 in 2x4 = 0.5, 1xk in 1x20 = k/20, ...)."""
import numpy as np

from isegmi import coco


def rect_poly(x0, y0, x1, y1):
    return [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]


def rect_mask(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), np.uint8)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 1
    return m


def star_poly(rng, cx, cy, r, n=None):
    n = int(rng.integers(3, 9)) if n is None else n
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.35, 1.0, n) * r
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).ravel().tolist()


def blob_mask(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(int(rng.integers(1, 4))):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(2, h / 2 + 2), rng.uniform(2, w / 2 + 2)
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
    return m.astype(np.uint8)


def _res(iid, cat, score, mask):
    ys, xs = np.nonzero(mask)
    box = [0.0, 0.0, 0.0, 0.0] if ys.size == 0 else [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
    return {"image_id": iid, "category_id": cat, "score": float(score), "bbox": box, "segmentation": coco.rle_encode(mask)}


# (inner w x h, outer w x h): the inner rectangle lies inside the outer one, IoU = inner / outer exactly
THRESHOLD_PAIRS = [((2, 2), (4, 2)), ((3, 2), (4, 2)), ((3, 1), (5, 1)), ((7, 1), (10, 1)), ((4, 1), (5, 1)), ((9, 1), (10, 1)),
                   ((11, 1), (20, 1)), ((13, 1), (20, 1)), ((17, 1), (20, 1)), ((19, 1), (20, 1))]


def make_dataset(seed, n_images=60, n_cats=6, big_every=7):
    """-> (gt dict, results list).  Categories 1 .. n_cats; category n_cats - 1 has only crowd gts, category n_cats has no gt at all."""
    rng = np.random.default_rng(seed)
    images, anns, results = [], [], []
    next_id = 0                                    # the first gt has id 0
    cats = [{"id": c, "name": "c%d" % c} for c in range(1, n_cats + 1)]
    score_pool = [0.9, 0.8, 0.8, 0.7, 0.5, 0.5, 0.5, 0.3]
    for iid in range(1, n_images + 1):
        big = iid % big_every == 0
        h, w = (int(rng.integers(110, 150)), int(rng.integers(110, 150))) if big else (int(rng.integers(24, 64)), int(rng.integers(24, 64)))
        images.append({"id": iid, "height": h, "width": w, "file_name": "%d.png" % iid})
        mode = iid % 10
        n_gt = 0 if mode == 3 else int(rng.integers(1, 6))
        gts = []
        for j in range(n_gt):
            cat = int(rng.integers(1, n_cats - 1))
            kind = int(rng.integers(0, 6))
            a = {"id": next_id, "image_id": iid, "category_id": cat, "iscrowd": 0}
            next_id += 1
            if kind == 0:       # integer rectangle polygon
                x0, y0 = int(rng.integers(0, w - 6)), int(rng.integers(0, h - 6))
                x1, y1 = int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))
                a["segmentation"] = [rect_poly(x0, y0, x1, y1)]
                mask = rect_mask(h, w, x0, y0, x1, y1)
                a["area"] = float((x1 - x0) * (y1 - y0))
            elif kind == 1:     # star polygon, possibly leaving the image; two parts now and then
                parts = [star_poly(rng, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(4, max(h, w) * (0.6 if big else 0.4)))]
                if rng.uniform() < 0.4:
                    parts.append(star_poly(rng, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(3, 12)))
                a["segmentation"] = parts
                mask = np.zeros((h, w), np.uint8)
                for p in parts:
                    mask |= coco.rle_decode({"size": [h, w], "counts": coco.rle_from_polygon(p, h, w)})
                if rng.uniform() < 0.5:
                    a["area"] = float(mask.sum()) + 0.5
            elif kind == 2:     # uncompressed RLE, no area, no bbox
                mask = blob_mask(rng, h, w)
                a["segmentation"] = {"size": [h, w], "counts": coco.rle_counts(mask)}
            elif kind == 3:     # compressed RLE with bbox
                mask = blob_mask(rng, h, w)
                a["segmentation"] = coco.rle_encode(mask)
                a["area"] = float(mask.sum())
                a["bbox"] = _res(iid, cat, 0, mask)["bbox"]
            elif kind == 4:     # crowd region
                mask = blob_mask(rng, h, w)
                a["segmentation"] = coco.rle_encode(mask); a["iscrowd"] = 1; a["area"] = float(mask.sum())
            else:               # empty mask, or an explicitly ignored gt
                if rng.uniform() < 0.5:
                    mask = np.zeros((h, w), np.uint8)
                    a["segmentation"] = coco.rle_encode(mask)
                else:
                    mask = blob_mask(rng, h, w)
                    a["segmentation"] = coco.rle_encode(mask); a["ignore"] = 1
            anns.append(a); gts.append((a, mask))
        if mode in (1, 5):      # crowd-only category
            mask = blob_mask(rng, h, w)
            a = {"id": next_id, "image_id": iid, "category_id": n_cats - 1, "iscrowd": 1, "segmentation": coco.rle_encode(mask), "area": float(mask.sum())}
            next_id += 1
            anns.append(a); gts.append((a, mask))
        if mode in (2, 6):      # a pair exactly on a threshold, in the small-area range, plus one identical det
            (iw, ih), (ow, oh) = THRESHOLD_PAIRS[(iid // 5) % len(THRESHOLD_PAIRS)]
            x0, y0 = int(rng.integers(0, w - ow)), int(rng.integers(0, h - oh))
            cat = 1 + iid % (n_cats - 2)
            a = {"id": next_id, "image_id": iid, "category_id": cat, "iscrowd": 0, "segmentation": [rect_poly(x0, y0, x0 + ow, y0 + oh)],
                 "area": float(ow * oh)}
            next_id += 1
            anns.append(a)
            results.append(_res(iid, cat, 0.8, rect_mask(h, w, x0, y0, x0 + iw, y0 + ih)))
            gts.append((a, rect_mask(h, w, x0, y0, x0 + ow, y0 + oh)))
        if mode == 4:           # an image with gts and no det
            continue
        for a, mask in gts:
            r = rng.uniform()
            sc = score_pool[int(rng.integers(0, len(score_pool)))]
            if r < 0.3:         # identical: IoU exactly 1.0 (0 for an empty mask)
                results.append(_res(iid, a["category_id"], sc, mask))
            elif r < 0.8:       # perturbed by a shift
                dy, dx = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
                results.append(_res(iid, a["category_id"], sc, np.roll(np.roll(mask, dy, 0), dx, 1)))
            if a["iscrowd"] and rng.uniform() < 0.7:    # several dets inside one crowd region
                for _ in range(3):
                    results.append(_res(iid, a["category_id"], score_pool[int(rng.integers(0, len(score_pool)))], mask & blob_mask(rng, h, w)))
        for _ in range(int(rng.integers(0, 4))):        # false positives, any category (also the one without gts), some empty
            cat = int(rng.integers(1, n_cats + 1))
            mask = blob_mask(rng, h, w) if rng.uniform() < 0.85 else np.zeros((h, w), np.uint8)
            results.append(_res(iid, cat, score_pool[int(rng.integers(0, len(score_pool)))], mask))
    return {"images": images, "categories": cats, "annotations": anns}, results
