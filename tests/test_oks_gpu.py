"""COCO keypoint evaluation on the MI355X: the OKS kernel (csrc/cocoeval.hip, isegmi_op_oks) against tests/oks_ref.py -- plain Python loops,
np.exp on scalars, terms added in index order -- and isegmi.cocoeval under "keypoints" end to end.

The one tolerance: |device - reference| <= (K + 2) * 2^-52.  The arguments of exp are bit-identical on both sides (the same IEEE double
operations in the same order, no contraction); the two math libraries document 1 ulp for exp, every term is <= 1 (1 ulp <= 2^-53 .. 2^-52), the
K - 1 additions and the division add at most 2^-53 each relative to a value <= K resp. <= 1.  The bound rests on that documentation, not on a
measurement; each test prints the largest difference it saw.  Everything downstream of OKS (matching, accumulate, the ten numbers) is compared
for equality: tests/oks_cases.py keeps every pair of the fixture away from the thresholds unless it sits exactly on one."""
import json
import os

import numpy as np
import pytest

import cocoeval_ref as ref
import oks_cases as cases
import oks_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bound(K):
    return (K + 2) * 2.0 ** -52


def _ref_pair(kp, box, area, var, d, g):
    return oks_ref.oks_pair(kp[d].ravel(), kp[g].ravel(), box[g], area[g], var)


@pytest.mark.parametrize("K", [1, 17, 32])
def test_oks_kernel_shapes(ffi, K):
    """15 gts and 20 dets; every [D][G] block form and every pair-list length, all against one reference matrix."""
    n_gt, n_dt = 15, 20
    kp, box, area, var = cases.kernel_items(100 + K, K, n_gt, n_dt)
    want = np.array([[_ref_pair(kp, box, area, var, n_gt + d, g) for g in range(n_gt)] for d in range(n_dt)], np.float64)
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() <= 1
    worst = 0.0
    for D, G in ((1, 1), (20, 1), (1, 15), (20, 15)):
        pairs = [(n_gt + d, g, 0) for d in range(D) for g in range(G)]           # row-major [D][G], as evaluate() sends a group
        got = ffi.oks(kp, box, area, var, pairs)
        assert got.dtype == np.float64 and got.shape == (D * G,) and np.isfinite(got).all()
        worst = max(worst, float(np.abs(got.reshape(D, G) - want[:D, :G]).max()))
    rng = np.random.default_rng(K)
    full = None
    for P in (0, 1, 63, 64, 65, 4097):
        dd, gg = rng.integers(0, n_dt, P), rng.integers(0, n_gt, P)
        pairs = np.stack([n_gt + dd, gg, rng.integers(0, 2, P)], 1) if P else np.zeros((0, 3), np.int32)   # the third column is not read
        got = ffi.oks(kp, box, area, var, pairs)
        assert got.shape == (P,)
        if P:
            worst = max(worst, float(np.abs(got - want[dd, gg]).max()))
        if P == 4097:
            full = (pairs, got)
    print("K = %d: largest |device - reference| = %.3g = %.2f * 2^-52 (bound %d * 2^-52)" % (K, worst, worst * 2.0 ** 52, K + 2))
    assert worst <= _bound(K)
    # determinism: the same call twice gives the same bytes; a pair alone gives what it gives inside the 4097-pair list, wherever it stands
    pairs, got = full
    assert ffi.oks(kp, box, area, var, pairs).tobytes() == got.tobytes()
    for j in (0, 63, 64, 255, 256, 4095, 4096):
        assert ffi.oks(kp, box, area, var, pairs[j:j + 1]).tobytes() == got[j:j + 1].tobytes(), j
    # the k1 == 0 gt (number 0) and the area-0 gt (number 1) are in the matrix; the first det coincides with the last gt where that is labelled
    if kp[n_gt - 1, :, 2].max() > 0:
        assert ffi.oks(kp, box, area, var, [(n_gt, n_gt - 1, 0)])[0] == 1.0


def test_oks_kernel_special_values(ffi):
    K = 5
    var = oks_ref.variances([0.05, 0.1, 0.025, 0.079, 0.107])
    items = []      # (keypoints [K][3], box, area)

    def item(xy, v, box=(0, 0, 1, 1), area=0.0):
        items.append((np.concatenate([np.asarray(xy, np.float64).reshape(K, 2), np.asarray(v, np.float64).reshape(K, 1)], 1), box, area))
        return len(items) - 1
    pts = [[10, 20], [30.5, 40.25], [50, 60], [70.125, 80], [90, 100]]
    far = lambda keep: [p if k in keep else [p[0] + 1e6, p[1] + 1e6] for k, p in enumerate(pts)]
    g_nan = item([pts[0], pts[1], [NAN, NAN], pts[3], [NAN, NAN]], [2, 1, 0, 2, 0], area=400.0)      # k1 = 3, NaN in the unlabelled slots
    d_same = item(pts, [0, 0, 0, 0, 0])                                                              # coincident; its v = 0 is never read
    d_near = item([[p[0] + 1.5, p[1] - 0.5] for p in pts], [1] * 5)
    g_none = item([[NAN, NAN]] * 5, [0] * 5, box=(10, 20, 30, 40), area=50.0)                        # k1 = 0: the doubled box is [-20, 70] x [-20, 100]
    d_in = item([[-20, -20], [70, 100], [0, 0], [69.5, 99.5], [25, 40]], [1] * 5)
    d_out = item([[73, 104], [70, 100], [0, 0], [-23, -24], [25, 40]], [1] * 5)
    g2 = item(pts, [2, 0, 0, 1, 0], area=3000.0); d2 = item(far({0}), [1] * 5)                       # k1 = 2, one coincident -> 1/2
    g4 = item(pts, [2, 1, 0, 1, 2], area=3000.0); d4 = item(far({0, 1, 3}), [1] * 5)                 # k1 = 4, three coincident -> 3/4
    g5 = item(pts, [2, 1, 1, 1, 2], area=9216.0); d5 = item(far({1, 2, 4}), [1] * 5)                 # k1 = 5, three coincident -> 3/5
    g_a0 = item(pts, [2, 2, 0, 0, 1], area=0.0)                                                      # area 0: the denominator is spacing(1)
    d_a0 = item([[10, 20], [30.5, 40.25], [0, 0], [0, 0], [90, 100.5]], [1] * 5)
    kp = np.stack([i[0] for i in items]); box = np.array([i[1] for i in items], np.float64); area = np.array([i[2] for i in items], np.float64)
    M = len(items)
    pairs = [(d_same, g_nan), (d_near, g_nan), (d_in, g_none), (d_out, g_none), (d2, g2), (d4, g4), (d5, g5), (d_same, g_a0), (d_a0, g_a0),
             (d_same, g5), (M, 0), (0, -1), (-1, M), (0, M), (2 ** 31 - 1, 0)]
    got = ffi.oks(kp, box, area, var, [(d, g, 0) for d, g in pairs])
    assert np.isfinite(got).all()
    assert got[0] == 1.0 and got[2] == 1.0 and got[9] == 1.0
    assert got[4] == 0.5 and got[5] == 0.75 and got[6] == 0.6
    assert got[7] == 1.0 and got[8] == 2.0 / 3.0          # area 0: coincident terms are exp(-0), the one 0.5 px off underflows to 0
    assert 0 < got[1] < 1 and 0 < got[3] < 1
    assert got[10:].tolist() == [-1.0] * 5
    want = np.array([_ref_pair(kp, box, area, var, d, g) for d, g in pairs[:10]])
    assert np.abs(got[:10] - want).max() <= _bound(K)
    # the arbiter agrees with both on these pairs
    for j in (1, 3):
        d, g = pairs[j]
        exact = oks_ref.oks_decimal(kp[d].ravel(), kp[g].ravel(), box[g], area[g], var)
        assert abs(float(exact) - got[j]) <= _bound(K) and abs(float(exact) - want[j]) <= _bound(K)
    with pytest.raises(ffi.IsegmiError):
        ffi.oks(np.zeros((2, 33, 3)), np.zeros((2, 4)), np.zeros(2), np.ones(33), [(0, 1, 0)])      # K beyond the engine's NUM_KEYPOINTS range


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def dataset():
    gt, res = cases.make_dataset(5)
    return gt, res, oks_ref.evaluate(gt, res, oks_ref.SIGMAS)


def _run(gt, res, budget=512 << 20):
    from isegmi import cocoeval
    e = cocoeval.COCOeval(cocoeval.COCOGt(gt), res, "keypoints", mem_budget=budget)
    e.evaluate(); e.accumulate(); e.summarize()
    return e


def test_end_to_end_equals_the_reference(ffi, dataset):
    gt, res, want = dataset
    e, small = _run(gt, res), _run(gt, res, 3 << 10)
    assert e.timings["chunks"] == 1 and small.timings["chunks"] > 10
    assert sorted(e.evalImgs) == sorted(want) == sorted(small.evalImgs)
    worst = 0.0
    for key, w in want.items():
        g, s = e.evalImgs[key], small.evalImgs[key]
        for name in ("dtScores", "dtMatches", "dtIgnore", "gtMatches", "gtIgnore"):
            assert np.array_equal(g[name], w[name]), (key, name)
        for name in ("dtScores", "dtMatches", "dtIgnore", "gtMatches", "gtIgnore", "ious"):
            assert g[name].tobytes() == s[name].tobytes() and g[name].shape == s[name].shape, (key, name)      # chunking changes nothing
        assert g["ious"].shape == w["ious"].shape
        if w["ious"].size:
            worst = max(worst, float(np.abs(g["ious"] - w["ious"]).max()))
            on = np.isin(w["ious"], cases.THRS) | (w["ious"] == 1.0) | (w["ious"] == 0.0)
            assert np.array_equal(g["ious"][on], w["ious"][on]), key          # on a threshold, exactly 0 and exactly 1: the same double on both sides
    print("fixture: largest |device - reference| OKS = %.3g = %.2f * 2^-52 (bound 19 * 2^-52)" % (worst, worst * 2.0 ** 52))
    assert worst <= _bound(17)
    p = e.params
    pr, rc, sc = ref.accumulate(want, 1, [20], 3, p.iouThrs, p.recThrs)
    stats = oks_ref.summarize(pr, rc, p.iouThrs)
    for run in (e, small):
        assert np.array_equal(run.eval["precision"], pr) and np.array_equal(run.eval["recall"], rc) and np.array_equal(run.eval["scores"], sc)
        assert run.stats.shape == (10,) and np.array_equal(run.stats, stats)
    assert e.summarize() == oks_ref.lines(stats)
    assert (stats > 0).all() and (stats < 1).all()


def test_perfect_results_score_one(ffi, dataset):
    """Detections = the gts' own keypoints: AP = AR = 1 (and both at .5 and .75) within the derived 1e-12 of the mask test.  The medium / large
    numbers need not be 1 -- there a detection whose own gt lies outside the range may take a gt inside it first, which is the matching rule at
    work, not an error -- so they are held against the reference instead, like all ten."""
    gt = dataset[0]
    res = cases.perfect_results(gt)
    e = _run(gt, res)
    assert e.stats.shape == (10,) and (np.abs(e.stats[[0, 1, 2, 5, 6, 7]] - 1.0) <= 1e-12).all(), e.stats
    p = e.params
    pr, rc, _ = ref.accumulate(oks_ref.evaluate(gt, res, oks_ref.SIGMAS), 1, [20], 3, p.iouThrs, p.recThrs)
    assert np.array_equal(e.stats, oks_ref.summarize(pr, rc, p.iouThrs))


def test_max_dets_is_twenty(ffi):
    """21 persons far apart and 21 detections, each a copy of one of them: the detection with the lowest score is cut and its person stays unmatched."""
    K = 17
    rng = np.random.default_rng(3)
    anns, res = [], []
    for j in range(21):
        kp = np.zeros((K, 3)); kp[:, 0] = 40 * j + rng.uniform(0, 20, K); kp[:, 1] = rng.uniform(0, 60, K); kp[:, 2] = 2
        kp = [float(v) for v in np.round(kp.ravel(), 2)]
        anns.append({"id": j + 1, "image_id": 1, "category_id": 1, "iscrowd": 0, "keypoints": kp, "num_keypoints": K, "bbox": [40.0 * j, 0.0, 20.0, 60.0],
                     "area": 1200.0})
        res.append({"image_id": 1, "category_id": 1, "keypoints": kp, "score": 0.9 - 0.01 * j})
    gt = {"images": [{"id": 1, "height": 100, "width": 900}], "categories": [{"id": 1, "name": "person"}], "annotations": anns}
    e = _run(gt, res)
    g = e.evalImgs[(0, 0)]
    assert g["dtMatches"].shape == (3, 10, 20) and g["ious"].shape == (20, 21)
    assert (g["dtMatches"][0] == np.arange(1, 21)).all() and (g["gtMatches"][0][:, :20] == np.arange(1, 21)).all() and not g["gtMatches"][:, :, 20].any()
    assert np.array_equal(e.eval["recall"][:, 0, 0, 0], np.full(10, 20 / 21))
    from isegmi import cocoeval
    stats = cocoeval.evaluate_results(gt, res, ("keypoints",))["keypoints"]
    assert stats.shape == (10,) and stats[5] == 20 / 21 and np.array_equal(stats, e.stats)


def test_evaluate_raises_by_name(ffi, dataset):
    from isegmi import cocoeval
    gt, res, _ = dataset
    bad = [dict(r) for r in res]
    bad[3]["keypoints"] = bad[3]["keypoints"][:48]
    with pytest.raises(ValueError, match=r"detection 4 has 48 keypoint numbers"):
        cocoeval.COCOeval(gt, bad, "keypoints").evaluate()
    bad = [dict(r) for r in res]
    del bad[0]["keypoints"]; bad[0]["bbox"] = [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError, match=r"detection 1 has no keypoints"):
        cocoeval.COCOeval(gt, bad, "keypoints").evaluate()
    g2 = dict(gt, annotations=[dict(a) for a in gt["annotations"]])
    del g2["annotations"][5]["bbox"]
    with pytest.raises(ValueError, match=r"ground truth %d has no bbox" % g2["annotations"][5]["id"]):
        cocoeval.COCOeval(g2, res, "keypoints").evaluate()
    g2 = dict(gt, annotations=[dict(a) for a in gt["annotations"]])
    g2["annotations"][5]["keypoints"] = g2["annotations"][5]["keypoints"] + [0, 0, 0]
    with pytest.raises(ValueError, match=r"ground truth %d has 54 keypoint numbers" % g2["annotations"][5]["id"]):
        cocoeval.COCOeval(g2, res, "keypoints").evaluate()
    g2 = dict(gt, annotations=[dict(a) for a in gt["annotations"]])
    del g2["annotations"][5]["keypoints"]
    with pytest.raises(ValueError, match=r"ground truth %d has no keypoints" % g2["annotations"][5]["id"]):
        cocoeval.COCOeval(g2, res, "keypoints").evaluate()
    e = cocoeval.COCOeval(gt, res, "keypoints")
    e.params.kpt_oks_sigmas = np.full(33, 0.05)
    with pytest.raises(ValueError, match="1 to 32"):
        e.evaluate()


def test_other_sigmas_and_keypoint_counts(ffi):
    """K = 3 with sigmas of the user's own, through COCOeval."""
    from isegmi import cocoeval
    sig = [0.05, 0.1, 0.025]
    gt, res = cases.make_dataset(9, n_images=6, K=3, sigmas=sig)
    e = cocoeval.COCOeval(gt, res, "keypoints")
    e.params.kpt_oks_sigmas = np.array(sig)
    e.evaluate()
    want = oks_ref.evaluate(gt, res, sig)
    for key, w in want.items():
        assert np.array_equal(e.evalImgs[key]["dtMatches"], w["dtMatches"]), key
        if w["ious"].size:
            assert np.abs(e.evalImgs[key]["ious"] - w["ious"]).max() <= _bound(3)


def test_keypoints_only_records_under_bbox(ffi, dataset):
    """A record with nothing but `keypoints` is evaluated under `bbox` with its extent box, as if the record carried that box."""
    from isegmi import cocoeval
    gt, res, _ = dataset
    assert any("bbox" not in r for r in res)
    spelled = [dict(r, bbox=oks_ref.extent(r["keypoints"])[1]) for r in res]
    a = cocoeval.evaluate_results(gt, res, ("bbox", "keypoints"))
    b = cocoeval.evaluate_results(gt, spelled, ("bbox", "keypoints"))
    assert a["bbox"].shape == (12,) and np.array_equal(a["bbox"], b["bbox"]) and np.array_equal(a["keypoints"], b["keypoints"])


def test_cli_coco_eval_keypoints(ffi, dataset, tmp_path, capsys):
    from isegmi import cli
    gt, res, _ = dataset
    (tmp_path / "gt.json").write_text(json.dumps(gt)); (tmp_path / "dt.json").write_text(json.dumps(res))
    out = tmp_path / "stats.json"
    cli.main(["coco_eval", "--gt", str(tmp_path / "gt.json"), "--dt", str(tmp_path / "dt.json"), "--iou-type", "keypoints", "--out", str(out)])
    e = _run(gt, res)
    assert json.loads(out.read_text()) == {"keypoints": [float(v) for v in e.stats]}
    printed = capsys.readouterr().out
    lines = e.summarize()
    assert len(lines) == 10 and "COCO keypoints evaluation:" in printed and all(l in printed for l in lines)


def test_engine_to_keypoint_score(ffi, tmp_path, capsys):
    """`test_net --gt` with the keypoint yaml on one image (the 128 x 160 canvas of tests/test_keypointrcnn_gpu.py) prints the bbox block and then
    the keypoints block.  A gt made from the engine's own results -- v = 2, the detection's box, area = box area -- scores keypoint AP 1; results
    with every keypoint shifted by half the box width score less."""
    from PIL import Image
    from conftest import ROOT
    from isegmi import cli, cocoeval
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(np.random.default_rng(20261019).integers(0, 256, (100, 130, 3)).astype(np.uint8)).save(src / "im0.png")
    person = {"id": 1, "image_id": 0, "category_id": 1, "iscrowd": 0, "bbox": [10.0, 10.0, 60.0, 80.0], "area": 4800.0,
              "keypoints": [float(v) for k in range(17) for v in (12 + 3 * k, 15 + 4 * k, 2)], "num_keypoints": 17}
    any_gt = {"images": [{"id": 0, "height": 100, "width": 130}], "categories": [{"id": 1, "name": "person"}], "annotations": [person]}
    (tmp_path / "gt.json").write_text(json.dumps(any_gt))
    results = cli.main(["test_net", "--config-file", os.path.join(ROOT, "configs", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml"), "--images", str(src),
                        "--output", str(tmp_path / "k.json"), "--batch_size", "1", "--gt", str(tmp_path / "gt.json"),
                        "MODEL.WEIGHT", "random", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "160", "MODEL.ROI_HEADS.SCORE_THRESH", "0.012"])
    printed = capsys.readouterr().out
    assert 0 <= printed.find("COCO bbox evaluation:") < printed.find("COCO keypoints evaluation:") and "COCO segm evaluation:" not in printed
    assert printed.count("Average Precision") == 6 + 5 and printed.count("Average Recall") == 6 + 5
    assert results and all(len(r["keypoints"]) == 51 and len(r["bbox"]) == 4 for r in results)
    results = sorted(results, key=lambda r: -r["score"])[:20]       # the keypoint evaluation looks at the 20 best detections of an image
    for k, r in enumerate(results):                                  # distinct scores, as in the mask test: a tie may swap two gts
        r["score"] = 1.0 - 1e-3 * k
    gt = dict(any_gt, annotations=[
        {"id": k + 1, "image_id": 0, "category_id": r["category_id"], "iscrowd": 0, "bbox": r["bbox"], "area": r["bbox"][2] * r["bbox"][3],
         "keypoints": [v if j % 3 < 2 else 2 for j, v in enumerate(r["keypoints"])], "num_keypoints": 17} for k, r in enumerate(results)])
    stats = cocoeval.evaluate_results(gt, results, ("bbox", "keypoints"))
    assert stats["bbox"].shape == (12,) and stats["keypoints"].shape == (10,)
    assert abs(stats["keypoints"][0] - 1.0) <= 1e-12 and abs(stats["keypoints"][5] - 1.0) <= 1e-12 and abs(stats["bbox"][0] - 1.0) <= 1e-12
    shifted = [dict(r, keypoints=[v + r["bbox"][2] / 2 if j % 3 == 0 else v for j, v in enumerate(r["keypoints"])]) for r in results]
    low = cocoeval.evaluate_results(gt, shifted, ("keypoints",))["keypoints"]
    assert low[0] < stats["keypoints"][0] - 0.05, low
