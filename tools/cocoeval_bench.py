#!/usr/bin/env python3
"""COCO evaluation timing on a seeded synthetic workload of COCO-val shape: 5000 images of 480 x 640, 80 categories, about 7 gts and up to 100
detections per image, masks of polygon-like size (convex blobs, 50 - 300 runs each).  Prints the time per stage of COCOeval.evaluate -- host
preparation (grouping, score sort), upload of the run counts, prefix kernel, IoU (pair list build + upload + kernel), matching (upload + kernel +
download) -- and of accumulate, plus the totals: one warm-up, then the median of --repeats runs.  There is no pass / fail time; the output is the record.

    python tools/cocoeval_bench.py [--images 5000] [--repeats 3] [--iou-type segm]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iou-type", dest="iou_type", default="segm", choices=["segm", "bbox"])
    a = ap.parse_args()
    from isegmi import _ffi, cocoeval
    assert _ffi.device_count() >= 1, "no HIP device"
    _ffi.set_device(0)
    t0 = time.perf_counter()
    gt_d, res = make(a.images)
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
    out = {"workload": {"images": a.images, "size": [H, W], "categories": 80, "gts": len(gt.anns), "dets": len(dt.anns),
                        "rle_runs": int(sum(len(x["counts"]) for x in gt.anns) + sum(len(x["counts"]) for x in dt.anns)),
                        "groups": int(med["groups"]), "pairs": int(med["pairs"]), "chunks": int(med["chunks"])},
           "iou_type": a.iou_type, "repeats": a.repeats, "generate_and_load_s": round(t_load, 3),
           "median_ms": {k: round(med[k] * 1e3, 2) for k in ("prepare", "upload", "prefix", "iou", "match", "evaluate", "accumulate", "total")},
           "spread_total_ms": [round(t["total"] * 1e3, 2) for t in runs], "AP": round(float(e.stats[0]), 4), "AP50": round(float(e.stats[1]), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
