#!/usr/bin/env python3
"""COCO evaluation timing on a seeded synthetic workload of COCO-val shape: 5000 images of 480 x 640, 80 categories, about 7 gts and up to 100
detections per image, masks of polygon-like size (convex blobs, 50 - 300 runs each).  Prints the time per stage of COCOeval.evaluate -- host
preparation (grouping, score sort), upload of the run counts, prefix kernel, IoU (pair list build + upload + kernel), matching (upload + kernel +
download) -- and of accumulate, plus the totals: one warm-up, then the median of --repeats runs.  There is no pass / fail time; the output is the record.

--iou-type keypoints takes a person-keypoint workload instead: one category, up to about 15 persons and up to 20 detections per image (jittered
copies of the persons plus unrelated ones), 17 keypoints.  The same run also times a plain numpy restatement of computeOks ([UPSTREAM-RECALL --
unverified]: one vectorised call per gt of a group, the terms added by np.sum) over the same groups, and reports how far the two differ.

    python tools/cocoeval_bench.py [--images 5000] [--repeats 3] [--iou-type segm|bbox|keypoints]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

H, W = 480, 640


def blob_counts(cx, cy, rx, ry):
    """Run counts of an axis-aligned ellipse clipped to the image: one run per column."""
    x = np.arange(max(int(cx - rx), 0), min(int(cx + rx) + 1, W))
    half = ry * np.sqrt(np.maximum(1.0 - ((x - cx) / rx) ** 2, 0.0))
    y0 = np.clip(np.floor(cy - half), 0, H).astype(np.int64); y1 = np.clip(np.ceil(cy + half), 0, H).astype(np.int64)
    ok = y1 > y0
    x, y0, y1 = x[ok], y0[ok], y1[ok]
    b = np.empty(2 * x.size + 1, np.int64)
    b[0:-1:2] = x * H + y0; b[1::2] = x * H + y1; b[-1] = H * W
    # a full-height column touches its neighbour: merge by dropping zero-length gaps
    c = np.diff(np.concatenate([[0], b]))
    if (c[1:] == 0).any():
        keep = [int(c[0])]
        j = 1
        while j < c.size:
            if c[j] > 0:
                keep.append(int(c[j])); j += 1
            else:
                j += 1
                if j < c.size:
                    keep[-1] += int(c[j]); j += 1
        return keep
    return c.tolist()


def make(n_images, seed=0):
    rng = np.random.default_rng(seed)
    images = [{"id": i, "height": H, "width": W} for i in range(1, n_images + 1)]
    cats = [{"id": c, "name": str(c)} for c in range(1, 81)]
    anns, res = [], []
    for i in range(1, n_images + 1):
        n_gt = int(rng.poisson(7))
        img_cats = rng.integers(1, 81, 4)
        shapes = []
        for _ in range(n_gt):
            s = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 120), rng.uniform(4, 120), int(img_cats[rng.integers(0, 4)]))
            shapes.append(s)
            c = blob_counts(*s[:4])
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": s[4], "iscrowd": int(rng.uniform() < 0.03),
                         "segmentation": {"size": [H, W], "counts": c}, "area": float(sum(c[1::2]))})
        n_dt = int(rng.integers(10, 101))
        for k in range(n_dt):
            if shapes and rng.uniform() < 0.6:      # a perturbed gt
                cx, cy, rx, ry, cat = shapes[int(rng.integers(0, len(shapes)))]
                s = (cx + rng.normal(0, 4), cy + rng.normal(0, 4), rx * rng.uniform(0.8, 1.2), ry * rng.uniform(0.8, 1.2), cat)
            else:
                s = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 120), rng.uniform(4, 120), int(img_cats[rng.integers(0, 4)]))
            res.append({"image_id": i, "category_id": s[4], "score": float(rng.uniform()), "segmentation": {"size": [H, W], "counts": blob_counts(*s[:4])}})
    return {"images": images, "categories": cats, "annotations": anns}, res


def make_keypoints(n_images, seed=0, K=17):
    """-> (annotation dict, result list) of the keypoint workload."""
    rng = np.random.default_rng(seed)
    images = [{"id": i, "height": H, "width": W} for i in range(1, n_images + 1)]
    anns, res = [], []
    for i in range(1, n_images + 1):
        persons = []
        for _ in range(min(int(rng.poisson(5)), 15)):
            bw, bh = rng.uniform(15, 200), rng.uniform(30, 400)
            bx, by = rng.uniform(0, W - 15), rng.uniform(0, H - 30)
            kp = np.zeros((K, 3)); kp[:, 0] = rng.uniform(bx, bx + bw, K); kp[:, 1] = rng.uniform(by, by + bh, K)
            kp[:, 2] = rng.choice([0, 1, 2], K, p=[0.3, 0.2, 0.5])
            kp[kp[:, 2] == 0, :2] = 0
            persons.append((kp, bw * bh * 0.5))
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": 1, "iscrowd": int(rng.uniform() < 0.03), "bbox": [bx, by, bw, bh],
                         "area": bw * bh * 0.5, "keypoints": kp.ravel().tolist(), "num_keypoints": int((kp[:, 2] > 0).sum())})
        for _ in range(int(rng.integers(0, 21))):
            kp = np.zeros((K, 3)); kp[:, 2] = 1
            if persons and rng.uniform() < 0.7:      # a jittered person
                g, area = persons[int(rng.integers(0, len(persons)))]
                kp[:, :2] = g[:, :2] + rng.normal(0, 1, (K, 2)) * rng.choice([0.01, 0.03, 0.1]) * np.sqrt(area)
            else:
                kp[:, 0] = rng.uniform(0, W, K); kp[:, 1] = rng.uniform(0, H, K)
            x0, y0 = kp[:, 0].min(), kp[:, 1].min()
            res.append({"image_id": i, "category_id": 1, "score": float(rng.uniform()), "keypoints": kp.ravel().tolist(),
                        "bbox": [x0, y0, kp[:, 0].max() - x0, kp[:, 1].max() - y0]})
    return {"images": images, "categories": [{"id": 1, "name": "person"}], "annotations": anns}, res


def numpy_oks(e, gt, dt):
    """[UPSTREAM-RECALL -- unverified] computeOks in plain numpy over the groups of a finished COCOeval `e` (its detection order and cut):
    per gt of a group one vectorised expression over the group's detections.  -> (seconds, {group key: [D][G] float64})."""
    ga = {a["id"]: a for a in gt.anns}
    da = {a["id"]: a for a in dt.anns}
    var = (np.asarray(e.params.kpt_oks_sigmas, np.float64) * 2) ** 2
    k = len(var)
    t0 = time.perf_counter()
    out = {}
    for key, g in e.evalImgs.items():
        gts = [ga[i] for i in g["gtIds"]]; dts = [da[i] for i in g["dtIds"]]
        ious = np.zeros((len(dts), len(gts)))
        if len(gts) and len(dts):
            d = np.array([q["keypoints"] for q in dts], np.float64)
            xd, yd = d[:, 0::3], d[:, 1::3]
            for j, q in enumerate(gts):
                gk = np.array(q["keypoints"], np.float64)
                xg, yg, vg = gk[0::3], gk[1::3], gk[2::3]
                k1 = np.count_nonzero(vg > 0)
                bb = q["bbox"]
                x0 = bb[0] - bb[2]; x1 = bb[0] + bb[2] * 2
                y0 = bb[1] - bb[3]; y1 = bb[1] + bb[3] * 2
                if k1 > 0:
                    dx = xd - xg; dy = yd - yg
                else:
                    z = np.zeros((len(dts), k))
                    dx = np.maximum(z, x0 - xd) + np.maximum(z, xd - x1); dy = np.maximum(z, y0 - yd) + np.maximum(z, yd - y1)
                ee = (dx ** 2 + dy ** 2) / var / (q["area"] + np.spacing(1)) / 2
                if k1 > 0:
                    ee = ee[:, vg > 0]
                ious[:, j] = np.sum(np.exp(-ee), axis=1) / ee.shape[1]
        out[key] = ious
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iou-type", dest="iou_type", default="segm", choices=["segm", "bbox", "keypoints"])
    a = ap.parse_args()
    kpt = a.iou_type == "keypoints"
    from isegmi import _ffi, cocoeval
    assert _ffi.device_count() >= 1, "no HIP device"
    _ffi.set_device(0)
    t0 = time.perf_counter()
    gt_d, res = make_keypoints(a.images) if kpt else make(a.images)
    gt = cocoeval.COCOGt(gt_d)
    dt = cocoeval.load_results(gt, res)
    t_load = time.perf_counter() - t0
    runs = []
    for r in range(a.repeats + 1):       # run 0 is the warm-up (code objects load, first allocations)
        e = cocoeval.COCOeval(gt, dt, a.iou_type)
        e.evaluate()
        t1 = time.perf_counter()
        e.accumulate()
        e.summarize()
        t = dict(e.timings); t["accumulate"] = time.perf_counter() - t1; t["evaluate"] = t.pop("total"); t["total"] = t["evaluate"] + t["accumulate"]
        if r:
            runs.append(t)
    med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
    out = {"workload": {"images": a.images, "size": [H, W], "categories": 1 if kpt else 80, "gts": len(gt.anns), "dets": len(dt.anns),
                        "rle_runs": 0 if kpt else int(sum(len(x["counts"]) for x in gt.anns) + sum(len(x["counts"]) for x in dt.anns)),
                        "groups": int(med["groups"]), "pairs": int(med["pairs"]), "chunks": int(med["chunks"])},
           "iou_type": a.iou_type, "repeats": a.repeats, "generate_and_load_s": round(t_load, 3),
           "median_ms": {k: round(med[k] * 1e3, 2) for k in ("prepare", "upload", "prefix", "iou", "match", "evaluate", "accumulate", "total")},
           "spread_total_ms": [round(t["total"] * 1e3, 2) for t in runs], "AP": round(float(e.stats[0]), 4), "AP50": round(float(e.stats[1]), 4)}
    if kpt:
        sizes = [g["ious"].shape for g in e.evalImgs.values()]
        out["workload"].update({"keypoints": len(e.params.kpt_oks_sigmas), "max_dets_per_group": max(s[0] for s in sizes),
                                "max_gts_per_group": max(s[1] for s in sizes)})
        secs, worst = [], 0.0
        for _ in range(a.repeats):
            s, host = numpy_oks(e, gt, dt)
            secs.append(s)
        for key, g in e.evalImgs.items():
            if g["ious"].size:
                worst = max(worst, float(np.abs(g["ious"] - host[key]).max()))
        out["numpy_oks_ms"] = round(float(np.median(secs)) * 1e3, 2)
        out["max_abs_diff_device_vs_numpy"] = worst
    print(json.dumps(out))


if __name__ == "__main__":
    main()
