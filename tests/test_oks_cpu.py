"""COCO keypoint evaluation without a GPU: KeypointParams, loading of keypoint records, hand-derived OKS values of the reference, the ten-line
summary, and the properties the GPU tests rely on in tests/oks_cases.py (margin from the thresholds, pairs exactly on them, discrimination)."""
import math

import numpy as np
import pytest

import cocoeval_ref as ref
import oks_cases as cases
import oks_ref
from isegmi import cocoeval


@pytest.fixture(scope="module")
def dataset():
    gt, res = cases.make_dataset(5)
    return gt, res, oks_ref.evaluate(gt, res, oks_ref.SIGMAS)


def test_keypoint_params_defaults():
    p = cocoeval.KeypointParams()
    assert isinstance(p, cocoeval.Params) and p.iouType == "keypoints"
    assert p.maxDets == [20] and p.useCats == 1
    assert p.areaRng == [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]] and p.areaRngLbl == ["all", "medium", "large"]
    assert np.array_equal(p.iouThrs, np.linspace(.5, .95, 10)) and np.array_equal(p.recThrs, np.linspace(0, 1, 101))
    assert np.array_equal(p.kpt_oks_sigmas, np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0)
    assert np.array_equal(p.kpt_oks_sigmas, oks_ref.SIGMAS) and np.allclose(p.kpt_oks_sigmas[:3], [.026, .025, .025], rtol=2.0 ** -51, atol=0)
    with pytest.raises(ValueError, match="KeypointParams"):
        cocoeval.Params("keypoints")
    gt = {"images": [{"id": 1, "height": 10, "width": 10}], "categories": [{"id": 1}], "annotations": []}
    assert isinstance(cocoeval.COCOeval(gt, [], "keypoints").params, cocoeval.KeypointParams)
    assert type(cocoeval.COCOeval(gt, [], "bbox").params) is cocoeval.Params


def test_load_results_extents_and_keypoints_only_records():
    gt = cocoeval.COCOGt({"images": [{"id": 7, "height": 100, "width": 100}], "categories": [{"id": 1}], "annotations": [
        {"id": 1, "image_id": 7, "category_id": 1, "bbox": [1, 2, 30, 40], "area": 600, "keypoints": [5, 6, 2, 0, 0, 0, 9, 8, 1]},
        {"id": 2, "image_id": 7, "category_id": 1, "bbox": [1, 2, 30, 40], "area": 600, "keypoints": [5, 6, 2, 0, 0, 0, 9, 8, 1], "num_keypoints": 3}]})
    assert gt.anns[0]["keypoints"] == [5, 6, 2, 0, 0, 0, 9, 8, 1] and gt.anns[0]["num_keypoints"] == 2     # absent: the count of v > 0
    assert gt.anns[1]["num_keypoints"] == 3                                                                 # present: kept as it is
    kp = [10.5, 20.0, 1, 40.0, 5.25, 0, 12.0, 60.0, 2]
    dt = cocoeval.load_results(gt, [{"image_id": 7, "category_id": 1, "score": 0.5, "keypoints": kp},
                                    {"image_id": 7, "category_id": 1, "score": 0.4, "keypoints": kp, "bbox": [0, 0, 50, 50]}])
    for r in dt.anns:                                         # v plays no part in the extents
        assert r["keypoints"] == kp and r["kp_area"] == (40.0 - 10.5) * (60.0 - 5.25) and r["kp_bbox"] == [10.5, 5.25, 29.5, 54.75]
    assert dt.anns[0]["bbox"] is None and dt.anns[1]["bbox"] == [0, 0, 50, 50]
    assert oks_ref.extent(kp) == (dt.anns[0]["kp_area"], dt.anns[0]["kp_bbox"])
    with pytest.raises(ValueError):
        cocoeval.load_results(gt, [{"image_id": 7, "category_id": 1, "score": 0.5}])
    with pytest.raises(ValueError, match="keypoints"):
        cocoeval.load_results(gt, [{"image_id": 7, "category_id": 1, "score": 0.5, "keypoints": [1, 2, 2, 3]}])


def test_reference_oks_hand_derived():
    var1 = oks_ref.variances([0.1])
    assert var1[0] == (np.float64(0.1) * 2) ** 2
    # one keypoint, d = (3, 4), sigma 0.1, area 100: e = 25 / 0.04 / 100 / 2 = 3.125 up to the rounding of 0.04 and of 100 + 2^-52
    idx, es = oks_ref.exp_args([13, 24, 1], [10, 20, 2], [0, 0, 5, 5], 100.0, var1)
    assert idx == [0] and abs(float(es[0]) - 3.125) <= 3.125 * 4 * 2.0 ** -52
    assert abs(oks_ref.oks_pair([13, 24, 1], [10, 20, 2], [0, 0, 5, 5], 100.0, var1) - math.exp(-3.125)) <= 8 * 2.0 ** -52
    # k1 == 0: box (10, 20, 30, 40) doubles to x in [-20, 70], y in [-20, 100].  Inside: every e is 0, OKS is exactly 1
    var2 = oks_ref.variances([0.1, 0.05])
    g0 = [0, 0, 0, 0, 0, 0]
    assert oks_ref.oks_pair([-20, 100, 1, 70, -20, 1], g0, [10, 20, 30, 40], 50.0, var2) == 1.0
    # outside: keypoint 0 at (73, 104) is (3, 4) beyond the corner, keypoint 1 inside -> (exp(-25 / 0.04 / 50 / 2) + 1) / 2
    v = oks_ref.oks_pair([73, 104, 1, 0, 0, 1], g0, [10, 20, 30, 40], 50.0, var2)
    assert abs(v - (math.exp(-6.25) + 1) / 2) <= 8 * 2.0 ** -52
    # left of / above the box: x0 - xd and y0 - yd take over
    v = oks_ref.oks_pair([-23, -24, 1, 0, 0, 1], g0, [10, 20, 30, 40], 50.0, var2)
    assert abs(v - (math.exp(-6.25) + 1) / 2) <= 8 * 2.0 ** -52
    # an unlabelled slot is selected out: NaN there changes nothing, and only k1 = 1 keypoint counts
    nan = float("nan")
    a = oks_ref.oks_pair([13, 24, 1, 500, 500, 1], [10, 20, 2, nan, nan, 0], [0, 0, 5, 5], 100.0, oks_ref.variances([0.1, 0.1]))
    assert a == oks_ref.oks_pair([13, 24, 1], [10, 20, 2], [0, 0, 5, 5], 100.0, var1)
    # the detection's v is not read; area 0 stays finite: coincident -> 1, apart -> 0
    assert oks_ref.oks_pair([13, 24, 0], [10, 20, 2], [0, 0, 5, 5], 100.0, var1) == oks_ref.oks_pair([13, 24, 2], [10, 20, 2], [0, 0, 5, 5], 100.0, var1)
    assert oks_ref.oks_pair([10, 20, 1], [10, 20, 2], [0, 0, 5, 5], 0.0, var1) == 1.0
    assert oks_ref.oks_pair([10, 21, 1], [10, 20, 2], [0, 0, 5, 5], 0.0, var1) == 0.0
    # the decimal arbiter agrees with the float route to the last bits
    d = oks_ref.oks_decimal([13, 24, 1], [10, 20, 2], [0, 0, 5, 5], 100.0, var1)
    assert abs(float(d) - oks_ref.oks_pair([13, 24, 1], [10, 20, 2], [0, 0, 5, 5], 100.0, var1)) <= 3 * 2.0 ** -52


def test_thresholds_hold_the_constructed_values():
    thr = np.linspace(.5, .95, 10)
    assert thr[0] == 0.5 and thr[5] == 0.75 and thr[2] == 0.6
    assert np.float64(1) / np.float64(2) == 0.5 and np.float64(3) / np.float64(4) == 0.75 and np.float64(3) / np.float64(5) == 0.6
    assert np.array_equal(cocoeval.KeypointParams().iouThrs, thr)


def test_ten_line_format_and_order():
    p = cocoeval.KeypointParams()
    T, R = len(p.iouThrs), len(p.recThrs)
    precision = -np.ones((T, R, 1, 3, 1)); recall = -np.ones((T, 1, 3, 1))
    for a in range(3):
        for t in range(T):
            precision[t, :, 0, a, 0] = 0.1 * (a + 1) + 0.01 * t
            recall[t, 0, a, 0] = 0.2 * (a + 1) + 0.02 * t
    stats, lines = cocoeval.summarize({"precision": precision, "recall": recall}, p)
    want = oks_ref.summarize(precision, recall, p.iouThrs)
    assert stats.shape == (10,) and np.array_equal(stats, want)
    assert abs(stats[1] - 0.1) < 1e-15 and abs(stats[2] - 0.15) < 1e-15 and abs(stats[4] - 0.345) < 1e-15 and abs(stats[8] - 0.49) < 1e-15
    assert lines == oks_ref.lines(want)
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 0.145"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets= 20 ] = 0.245"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50      | area=   all | maxDets= 20 ] = 0.200"
    assert lines[9] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets= 20 ] = 0.690"
    recall[:, :, 2, :] = -1                                   # a range without any gt prints -1
    assert cocoeval.summarize({"precision": precision, "recall": recall}, p)[0][9] == -1.0


def test_index_order_sum_against_np_sum(dataset):
    """The stated order against upstream's np.sum: K terms <= 1, so either sum carries at most (K - 1) roundings of at most 2^-53 * K each."""
    gt, res, _ = dataset
    K = 17
    var = oks_ref.variances(oks_ref.SIGMAS)
    by_img = {}
    for a in gt["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    worst, differ = 0.0, 0
    for r in res:
        for g in by_img.get(r["image_id"], []):
            a, b = oks_ref.oks_pair(r["keypoints"], g["keypoints"], g["bbox"], g["area"], var), \
                oks_ref.oks_np_sum(r["keypoints"], g["keypoints"], g["bbox"], g["area"], var)
            worst = max(worst, abs(a - b)); differ += a != b
    print("index order vs np.sum: largest difference %.3g, %d pairs differ" % (worst, differ))
    assert worst <= (K - 1) * 2.0 ** -52 * K


def test_generator_contents_and_margin(dataset):
    gt, res, want = dataset
    anns = gt["annotations"]
    assert 35 <= len(gt["images"]) <= 45 and len({(im["height"], im["width"]) for im in gt["images"]}) > 30
    n_gt, n_dt = {}, {}
    for a in anns:
        n_gt[a["image_id"]] = n_gt.get(a["image_id"], 0) + 1
    for r in res:
        n_dt[r["image_id"]] = n_dt.get(r["image_id"], 0) + 1
    assert max(n_gt.values()) == 15 and max(n_dt.values()) > 20 and max(n_dt.values()) <= 25
    assert any(i not in n_dt for i in n_gt) and any(i not in n_gt for i in n_dt)               # gts without detections and the reverse
    assert any(a["iscrowd"] for a in anns)
    none = [a for a in anns if a["num_keypoints"] == 0]
    assert none and all(not any(a["keypoints"]) and a["bbox"][2] > 0 for a in none)
    assert any(a["num_keypoints"] == 1 for a in anns)
    vs = {v for a in anns for v in a["keypoints"][2::3]}
    assert vs == {0, 1, 2}
    areas = [a["area"] for a in anns]
    assert 0.0 in areas and 1024.0 in areas and 9216.0 in areas
    assert any(0 < v < 1024 for v in areas) and any(1024 < v < 9216 for v in areas) and any(v > 9216 for v in areas)
    scores = [r["score"] for r in res]
    assert len(set(scores)) < len(scores)
    assert any("bbox" not in r for r in res) and any("bbox" in r for r in res)
    assert any(v == 0 for r in res for v in r["keypoints"][2::3])
    # the margin: no reference OKS is near a threshold without being on it; the constructed values are there, and so is an exact 1
    allv = np.concatenate([e["ious"].ravel() for e in want.values()])
    assert allv.size > 2000 and np.isfinite(allv).all() and allv.min() >= 0 and allv.max() == 1.0
    for t in cases.THRS:
        near = np.abs(allv - t) <= cases.MARGIN
        assert (allv[near] == t).all()
    for _, _, v in cases.ON_THRESHOLD:
        assert (allv == v).any(), v
    assert (allv > 0.5).sum() > 100 and (allv < 0.5).sum() > 100
    cut = [e for e in want.values() if len(e["dtScores"]) == 20]
    assert cut                                                  # the cut at 20 bites


def test_fixture_discriminates(dataset):
    """Three plausible mistakes each change some reference value on this fixture: reading the detection's v, dividing by K instead of k1,
    dropping spacing(1) from the denominator."""
    gt, res, want = dataset
    base = np.concatenate([e["ious"].ravel() for e in want.values()])
    for variant in ("det_v", "div_K", "no_eps"):
        other = np.concatenate([e["ious"].ravel() for e in oks_ref.evaluate(gt, res, oks_ref.SIGMAS, variant=variant).values()])
        assert not np.array_equal(base, other, equal_nan=True), variant


def test_reference_end_to_end_is_sane(dataset):
    gt, res, want = dataset
    p = cocoeval.KeypointParams()
    pr, rc, sc = ref.accumulate(want, 1, [20], 3, p.iouThrs, p.recThrs)
    stats = oks_ref.summarize(pr, rc, p.iouThrs)
    assert (stats > 0).all() and (stats < 1).all() and stats[1] >= stats[0] >= 0 and stats[6] >= stats[5]


def test_cli_parser_accepts_keypoints():
    from isegmi import cli
    a = cli.build_parser().parse_args(["coco_eval", "--gt", "g.json", "--dt", "d.json", "--iou-type", "keypoints"])
    assert a.iou_type == "keypoints"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["coco_eval", "--gt", "g.json", "--dt", "d.json", "--iou-type", "oks"])
