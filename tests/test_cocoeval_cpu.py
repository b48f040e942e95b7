"""Host side of COCO evaluation (isegmi.coco polygon / merge restatements, isegmi.cocoeval accumulate / summarize, CLI surface) on the CPU.
The device half (IoU, matching) is replaced here by tests/cocoeval_ref.py's match arrays; tests/test_cocoeval_gpu.py covers it."""
import numpy as np
import pytest

import cocoeval_data as data
import cocoeval_ref as ref
from isegmi import coco


def _poly_mask(xy, h, w):
    return coco.rle_decode({"size": [h, w], "counts": coco.rle_from_polygon(xy, h, w)}).astype(bool)


def test_polygon_integer_rectangles_are_exact():
    rng = np.random.default_rng(0)
    for _ in range(200):
        h, w = int(rng.integers(2, 70)), int(rng.integers(2, 90))
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))
        c = coco.rle_from_polygon(data.rect_poly(x0, y0, x1, y1), h, w)
        assert sum(c) == h * w and all(v > 0 for v in c[1:])
        assert np.array_equal(_poly_mask(data.rect_poly(x0, y0, x1, y1), h, w), data.rect_mask(h, w, x0, y0, x1, y1).astype(bool)), (h, w, x0, y0, x1, y1)
        assert coco.rle_area(c) == (x1 - x0) * (y1 - y0)
        assert coco.rle_to_bbox(c, h) == [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]


def _even_odd(px, py, xy):
    """fp64 even-odd point-in-polygon of the points (px, py)."""
    x, y = np.asarray(xy[0::2], np.float64), np.asarray(xy[1::2], np.float64)
    inside = np.zeros(px.shape, bool)
    for j in range(len(x)):
        xa, ya, xb, yb = x[j], y[j], x[(j + 1) % len(x)], y[(j + 1) % len(x)]
        if ya == yb:
            continue
        cross = ((ya > py) != (yb > py)) & (px < (xb - xa) * (py - ya) / (yb - ya) + xa)
        inside ^= cross
    return inside


def _chebyshev_to_edges(px, py, xy):
    """Smallest L-infinity distance from every point to the polygon's edges.  max(|f|, |g|) of two linear functions of the edge parameter
    is convex and piecewise linear: its minimum over [0, 1] is at an end or where f = 0, g = 0, f = g or f = -g."""
    x, y = np.asarray(xy[0::2], np.float64), np.asarray(xy[1::2], np.float64)
    best = np.full(px.shape, np.inf)
    for j in range(len(x)):
        ax, ay = x[j], y[j]
        ux, uy = x[(j + 1) % len(x)] - ax, y[(j + 1) % len(x)] - ay
        fx, fy = ax - px, ay - py                       # f(t) = fx + t ux, g(t) = fy + t uy
        cands = [np.zeros(px.shape), np.ones(px.shape)]
        with np.errstate(divide="ignore", invalid="ignore"):
            for num, den in ((-fx, ux), (-fy, uy), (fy - fx, ux - uy), (-fx - fy, ux + uy)):
                t = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0) if np.ndim(den) else (num / den if den != 0 else np.zeros(px.shape))
                cands.append(np.clip(t, 0.0, 1.0))
        for t in cands:
            best = np.minimum(best, np.maximum(np.abs(fx + t * ux), np.abs(fy + t * uy)))
    return best


def test_polygon_agrees_with_point_in_polygon_outside_a_one_pixel_band():
    """Condition, not measurement: every pixel whose centre is more than 1 px (Chebyshev) from every edge must agree with the fp64 even-odd test
    at the centre.  Star polygons are simple (vertices sorted by angle around one centre), convex and concave."""
    rng = np.random.default_rng(1)
    h, w = 60, 80
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx + 0.5, yy + 0.5
    checked = 0
    for k in range(120):
        xy = data.star_poly(rng, rng.uniform(10, w - 10), rng.uniform(10, h - 10), rng.uniform(5, 30))
        got = _poly_mask(xy, h, w)
        far = _chebyshev_to_edges(px, py, xy) > 1.0
        want = _even_odd(px, py, xy)
        assert np.array_equal(got[far], want[far]), (k, np.argwhere(far & (got != want))[:4])
        checked += int(far.sum())
    assert checked > 100000


def test_polygon_leaving_the_image_is_clipped():
    h, w = 20, 30
    m = _poly_mask([-10, -10, 50, -10, 50, 40, -10, 40], h, w)
    assert m.all()
    m = _poly_mask([-5.0, 5.0, 10.0, 5.0, 10.0, 100.0, -5.0, 100.0], h, w)
    assert np.array_equal(m, data.rect_mask(h, w, 0, 5, 10, h).astype(bool))
    rng = np.random.default_rng(2)
    for _ in range(50):
        xy = data.star_poly(rng, rng.uniform(-10, w + 10), rng.uniform(-10, h + 10), rng.uniform(5, 60))
        c = coco.rle_from_polygon(xy, h, w)
        assert sum(c) == h * w and min(c) >= 0


def test_merge_and_area_equal_the_dense_union():
    rng = np.random.default_rng(3)
    for _ in range(60):
        h, w = int(rng.integers(1, 50)), int(rng.integers(1, 50))
        masks = [data.blob_mask(rng, h, w) if rng.uniform() < 0.8 else np.zeros((h, w), np.uint8) for _ in range(int(rng.integers(1, 5)))]
        if rng.uniform() < 0.2:
            masks.append(np.ones((h, w), np.uint8))
        u = coco.rle_merge([coco.rle_counts(m) for m in masks], h * w)
        want = np.zeros((h, w), bool)
        for m in masks:
            want |= m.astype(bool)
        assert u == coco.rle_counts(want), (h, w)            # canonical: the very counts the encoder gives for the union
        assert coco.rle_area(u) == int(want.sum())
        assert coco.rle_to_bbox(u, h) == ref.tight_box(want)


def _ref_eval(gt, res, iou_type, params):
    return ref.evaluate(gt, res, iou_type, [im["id"] for im in gt["images"]], [c["id"] for c in gt["categories"]], params.useCats,
                        params.maxDets, params.areaRng, params.iouThrs)


def _params(gt, iou_type="segm"):
    from isegmi import cocoeval
    p = cocoeval.Params(iou_type)
    p.imgIds = [im["id"] for im in gt["images"]]
    p.catIds = [c["id"] for c in gt["categories"]]
    return p


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_accumulate_and_summarize_equal_the_reference(iou_type):
    from isegmi import cocoeval
    gt, res = data.make_dataset(11, n_images=80)
    p = _params(gt, iou_type)
    ev = _ref_eval(gt, res, iou_type, p)
    got = cocoeval.accumulate(ev, p)
    pr, rc, sc = ref.accumulate(ev, len(p.catIds), p.maxDets, len(p.areaRng), p.iouThrs, p.recThrs)
    assert got["precision"].dtype == np.float64
    assert np.array_equal(got["precision"], pr) and np.array_equal(got["recall"], rc) and np.array_equal(got["scores"], sc)
    assert (pr == -1).any() and (pr > 0).any()
    stats, lines = cocoeval.summarize(got, p)
    assert np.array_equal(stats, ref.summarize(pr, rc, p.iouThrs, p.maxDets))
    assert len(lines) == 12 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[0]
    assert lines[8].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")


def _stats(gt, res):
    from isegmi import cocoeval
    p = _params(gt)
    ev = cocoeval.accumulate(_ref_eval(gt, res, "segm", p), p)
    return cocoeval.summarize(ev, p)[0], ev


def _small_gt(h=40, w=50, second_image=2):
    """Three images with one gt each (two images when second_image = 1): category 1 with small (area 12, 20) and medium (35 x 35) gts,
    category 2 without any gt."""
    rects = [(1, 2, 3, 6, 6), (second_image, 10, 10, 15, 14), (3, 1, 1, 36, 36)]
    anns = [{"id": k, "image_id": i, "category_id": 1, "iscrowd": 0, "segmentation": [data.rect_poly(x0, y0, x1, y1)],
             "area": float((x1 - x0) * (y1 - y0))} for k, (i, x0, y0, x1, y1) in enumerate(rects)]
    gt = {"images": [{"id": i, "height": h, "width": w} for i in (1, 2, 3)],
          "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}], "annotations": anns}
    return gt, rects


def test_perfect_detections_score_one():
    gt, rects = _small_gt()
    res = [data._res(i, 1, 0.9 - 0.1 * k, data.rect_mask(40, 50, x0, y0, x1, y1)) for k, (i, x0, y0, x1, y1) in enumerate(rects)]
    stats, ev = _stats(gt, res)
    # spacing(1) in the precision denominator keeps a perfect precision one ulp under 1: compare within 1e-12, not ==
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
        assert abs(stats[k] - 1.0) <= 1e-12, (k, stats[k])
    assert stats[5] == -1 and stats[11] == -1          # no gt of large size
    assert (ev["precision"][:, :, 1] == -1).all() and (ev["recall"][:, 1] == -1).all()   # the category with no gt


def test_perfect_recall_at_one_det_counts_gts_over_the_category():
    """maxDets = 1 keeps one det per image: 2 of the 3 gts are found, recall 2 / 3 (written out: images pool inside a category)."""
    gt, rects = _small_gt(second_image=1)
    res = [data._res(i, 1, 0.9, data.rect_mask(40, 50, x0, y0, x1, y1)) for (i, x0, y0, x1, y1) in rects]
    stats, _ = _stats(gt, res)
    assert abs(stats[6] - 2.0 / 3.0) <= 1e-12


def test_no_detections_score_zero():
    gt, _ = _small_gt()
    stats, ev = _stats(gt, [])
    assert [stats[k] for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)] == [0.0] * 10 and stats[5] == -1 and stats[11] == -1
    assert (ev["precision"][:, :, 1] == -1).all()


def test_three_detections_hand_computed_ap50():
    """One image, 2 gts; dets 0.9 (TP), 0.8 (FP), 0.7 (TP).  Sorted by score: tp = 1, 1, 2; fp = 0, 1, 1; recall = 0.5, 0.5, 1.0;
    precision = 1, 1/2, 2/3 -> running maximum from the back: 1, 2/3, 2/3.  recThrs 0 .. 0.50 (51 values) take the first entry with
    recall >= thr: index 0, precision 1; recThrs 0.51 .. 1.00 (50 values) take index 2, precision 2/3.
    AP@0.5 = (51 * 1 + 50 * 2/3) / 101.  The same at every threshold (all IoUs are 1.0 or 0.0), so AP = AP50 = AP75."""
    h, w = 40, 50
    gt = {"images": [{"id": 7, "height": h, "width": w}], "categories": [{"id": 3, "name": "x"}],
          "annotations": [{"id": 0, "image_id": 7, "category_id": 3, "iscrowd": 0, "segmentation": [data.rect_poly(2, 2, 8, 8)], "area": 36.0},
                          {"id": 1, "image_id": 7, "category_id": 3, "iscrowd": 0, "segmentation": [data.rect_poly(20, 20, 30, 30)], "area": 100.0}]}
    res = [data._res(7, 3, 0.7, data.rect_mask(h, w, 20, 20, 30, 30)), data._res(7, 3, 0.9, data.rect_mask(h, w, 2, 2, 8, 8)),
           data._res(7, 3, 0.8, data.rect_mask(h, w, 40, 2, 45, 8))]
    stats, ev = _stats(gt, res)
    want = (51 * 1.0 + 50 * (2.0 / 3.0)) / 101
    assert abs(stats[1] - want) <= 1e-12 and abs(stats[0] - want) <= 1e-12 and abs(stats[2] - want) <= 1e-12
    assert abs(stats[8] - 1.0) <= 1e-12 and abs(stats[6] - 0.5) <= 1e-12
    p50 = ev["precision"][0, :, 0, 0, 2]
    assert np.all(np.abs(p50[:51] - 1.0) <= 1e-12) and np.all(np.abs(p50[51:] - 2.0 / 3.0) <= 1e-12)


def test_gt_and_results_loading():
    from isegmi import cocoeval
    gt, res = data.make_dataset(5, n_images=30)
    G = cocoeval.COCOGt(gt)
    imgs = {im["id"]: im for im in gt["images"]}
    assert G.anns[0]["id"] == 0
    for a, r in zip(gt["annotations"], G.anns):
        im = imgs[a["image_id"]]
        m = ref.seg_dense(a["segmentation"], im["height"], im["width"])
        assert np.array_equal(ref.dense(r["counts"], *r["size"]), m)
        assert r["area"] == (float(a["area"]) if "area" in a else float(m.sum()))
        assert r["bbox"] == ([float(v) for v in a["bbox"]] if "bbox" in a else ref.tight_box(m))
    dt = cocoeval.load_results(G, res)
    assert [d["id"] for d in dt.anns] == list(range(1, len(res) + 1))
    for a, r in zip(res, dt.anns):
        m = ref.seg_dense(a["segmentation"], 0, 0)
        assert r["seg_area"] == float(m.sum()) and r["seg_bbox"] == ref.tight_box(m) and r["bbox"] == a["bbox"]
    with pytest.raises(ValueError, match="not in the annotation file"):
        cocoeval.load_results(G, [dict(res[0], image_id=10 ** 6)])
    p = cocoeval.Params("bbox")
    assert list(p.maxDets) == [1, 10, 100] and len(p.iouThrs) == 10 and len(p.recThrs) == 101 and p.useCats == 1
    assert p.iouThrs[0] == 0.5 and p.recThrs[50] == 0.5 and p.areaRngLbl == ["all", "small", "medium", "large"]
    assert p.areaRng == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    with pytest.raises(ValueError):
        cocoeval.Params("keypoints")


def test_cli_surface():
    from isegmi import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["coco_eval", "--help"])
    assert e.value.code == 0
    ap = cli.build_parser()
    a = ap.parse_args(["coco_eval", "--gt", "a.json", "--dt", "r.json", "--iou-type", "bbox", "--cat-ids", "1", "3", "--max-dets", "1", "5"])
    assert a.gt == "a.json" and a.dt == "r.json" and a.iou_type == "bbox" and a.cat_ids == [1, 3] and a.max_dets == [1, 5] and a.out is None
    # the three existing commands keep their defaults; --gt is off unless given
    e = vars(ap.parse_args(["eval"]))
    assert e == {"cmd": "eval", "trained_model": "random", "config": "yolact_resnet50_config", "score_threshold": 0.0, "top_k": 5, "image": None,
                 "images": None, "output_coco_json": None, "batch_size": 8, "gt": None}
    t = vars(ap.parse_args(["test_net"]))
    assert t == {"cmd": "test_net", "config_file": "", "images": None, "output": "results.json", "batch_size": 2, "group": "canvas", "opts": [],
                 "gt": None}
    q = vars(ap.parse_args(["pose2seg_test", "--anno", "k.json", "--image-root", "d"]))
    assert q == {"cmd": "pose2seg_test", "weights": "random", "anno": "k.json", "image_root": "d", "output": "segm.json", "batch_size": 8,
                 "max_instances": 32, "gt": None}
