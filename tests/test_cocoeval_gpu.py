"""COCO evaluation on the MI355X: the mask-IoU, box-IoU and matching kernels (csrc/cocoeval.hip) against tests/cocoeval_ref.py -- dense boolean
planes and plain Python loops -- and isegmi.cocoeval end to end.  Everything is integer work plus single correctly rounded double operations in a
stated order, so every comparison is an equality; the one tolerance is the derived 1e-12 on AP = 1 (spacing(1) in the precision denominator)."""
import numpy as np
import pytest

import cocoeval_data as data
import cocoeval_ref as ref
from isegmi import coco

pytestmark = pytest.mark.gpu


def _iou_case(ffi, masks, pairs):
    """masks: list of equal-size uint8 planes per entry of `sizes`; pairs over the flat list."""
    rles = ffi.RleSet([coco.rle_counts(m) for m in masks], [m.shape for m in masks])
    assert np.array_equal(rles.area, np.array([int(m.sum()) for m in masks], np.int64))        # areas from the RLEs = dense pixel counts
    for k, m in enumerate(masks):
        x, y, w, h = ref.tight_box(m)
        want = [0, 0, -1, -1] if w == 0 else [int(x), int(y), int(x + w - 1), int(y + h - 1)]
        assert rles.bbox[k].tolist() == want, (k, rles.bbox[k], want)
    got = ffi.rle_iou(rles, pairs)
    want = np.array([ref.mask_iou(masks[d].astype(bool), masks[g].astype(bool), c) for d, g, c in pairs], np.float64)
    assert got.dtype == np.float64 and np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    rles.free()
    return got


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 64), (65, 63), (200, 257), (480, 640), (1500, 2000)])
def test_rle_iou_bitexact_shapes(ffi, h, w):
    rng = np.random.default_rng(h * 7 + w)
    check = np.add.outer(np.arange(h), np.arange(w)) % 2
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), check.astype(np.uint8), (1 - check).astype(np.uint8),       # 1 run .. h*w runs
             (rng.uniform(size=(h, w)) < 0.5).astype(np.uint8), data.blob_mask(rng, h, w), data.blob_mask(rng, h, w),
             data.rect_mask(h, w, 0, 0, max(w // 3, 1), max(h // 3, 1)), data.rect_mask(h, w, w - max(w // 3, 1), h - max(h // 3, 1), w, h)]
    m = data.blob_mask(rng, h, w); masks += [m, np.roll(m, 1, 0), m.copy()]
    last = np.zeros((h, w), np.uint8); last[-1, -1] = 1; first = np.zeros((h, w), np.uint8); first[0, 0] = 1
    masks += [last, first]
    n = len(masks)
    pairs = [(d, g, c) for d in range(n) for g in range(n) for c in (0, 1)]
    got = _iou_case(ffi, masks, pairs)
    assert got[pairs.index((9, 11, 0))] == 1.0 and got[pairs.index((0, 0, 0))] == 0.0


def test_rle_iou_generator_pairs_and_mixed_sizes(ffi):
    """The generator's own (det, gt) pairs: polygons, crowd regions, empty masks, pairs exactly on a threshold; images of different sizes in one set."""
    gt, res = data.make_dataset(21, n_images=60)
    imgs = {im["id"]: im for im in gt["images"]}
    masks, owner, crowd = [], [], []
    for a in gt["annotations"]:
        masks.append(ref.seg_dense(a["segmentation"], imgs[a["image_id"]]["height"], imgs[a["image_id"]]["width"]).astype(np.uint8))
        owner.append(a["image_id"]); crowd.append(a["iscrowd"])
    ng = len(masks)
    for r in res:
        masks.append(ref.seg_dense(r["segmentation"], 0, 0).astype(np.uint8)); owner.append(r["image_id"])
    pairs = [(d, g, crowd[g]) for d in range(ng, len(masks)) for g in range(ng) if owner[d] == owner[g]]
    got = _iou_case(ffi, masks, pairs)
    assert (got == 1.0).any() and (got == 0.0).any() and any((got == t).any() for t in (0.5, 0.75))
    # a pair of different sizes or an index out of range is flagged, not evaluated
    a, b = next((d, g) for d in range(len(masks)) for g in range(len(masks)) if masks[d].shape != masks[g].shape)
    rles = ffi.RleSet([coco.rle_counts(m) for m in masks], [m.shape for m in masks])
    assert ffi.rle_iou(rles, [(a, b, 0), (len(masks), 0, 0), (0, -1, 0)]).tolist() == [-1.0, -1.0, -1.0]
    rles.free()


def test_bbox_iou_bitexact(ffi):
    rng = np.random.default_rng(4)
    boxes = np.concatenate([rng.uniform(0, 100, (200, 4)), np.round(rng.uniform(0, 50, (100, 4)) * 10) / 10,
                            [[10, 10, 0, 5], [10, 10, 5, 0], [0, 0, 0, 0],            # degenerate: zero width / height / both
                             [0, 0, 10, 10], [10, 0, 10, 10], [0, 10, 10, 10],         # touching at an edge
                             [0, 0, 10, 10], [5, 5, 10, 10], [1e-3, 1e-3, 1e6, 1e6]]]).astype(np.float64)
    n = len(boxes)
    pairs = [(int(d), int(g), int(c)) for d, g, c in zip(rng.integers(0, n, 20000), rng.integers(0, n, 20000), rng.integers(0, 2, 20000))]
    pairs += [(d, g, c) for d in range(300, n) for g in range(300, n) for c in (0, 1)]
    got = ffi.bbox_iou(boxes, pairs)
    with np.errstate(all="ignore"):
        want = np.array([ref.bbox_iou(boxes[d], boxes[g], c) for d, g, c in pairs], np.float64)
    assert np.array_equal(got, want, equal_nan=True), np.nonzero(got != want)[0][:8]
    assert got[pairs.index((303, 304, 0))] == 0.0 and got[pairs.index((306, 307, 0))] == 25.0 / 175.0


def _match_both(ffi, groups, area_rng, iou_thrs):
    """groups: list of (ious [D][G], det_area, gt_area, gt_crowd, gt_ignore)."""
    det_off, gt_off, iou_off, flat = [0], [0], [], []
    for ious, da, ga, gc, gi in groups:
        iou_off.append(len(flat)); flat += [float(v) for row in ious for v in row]
        det_off.append(det_off[-1] + len(da)); gt_off.append(gt_off[-1] + len(ga))
    cat = lambda k, dt: np.array([v for g in groups for v in g[k]], dt)
    got = ffi.coco_match(det_off, gt_off, iou_off, np.array(flat, np.float64), cat(1, np.float64), cat(2, np.float64), cat(3, np.uint8),
                         cat(4, np.uint8), area_rng, iou_thrs)
    for j, (ious, da, ga, gc, gi) in enumerate(groups):
        want = ref.match_group(ious, da, ga, gc, gi, area_rng, iou_thrs)
        d0, d1, g0, g1 = det_off[j], det_off[j + 1], gt_off[j], gt_off[j + 1]
        assert np.array_equal(got[0][:, :, d0:d1], want[0]), ("dtMatches", j, got[0][:, :, d0:d1], want[0])
        assert np.array_equal(got[1][:, :, d0:d1], want[1]), ("dtIgnore", j)
        assert np.array_equal(got[2][:, :, g0:g1], want[2]), ("gtMatches", j)
        assert np.array_equal(got[3][:, g0:g1], want[3]), ("gtIgnore", j)
    return got


def test_coco_match_crafted_cases(ffi):
    from isegmi.cocoeval import Params
    p = Params("segm")
    rng, thr = p.areaRng, p.iouThrs
    groups = [
        # a crowd gt (index 1) matched by several dets; the plain gt 0 only once
        ([[0.9, 0.8], [0.85, 0.7], [0.2, 0.6], [0.1, 0.95]], [50, 50, 50, 50], [100, 400], [0, 1], [0, 0]),
        # an ignored gt (explicit flag, index 0 -- it is visited LAST) with the higher IoU follows a held match on gt 1: the scan stops before it
        ([[0.95, 0.6], [0.9, 0.2]], [50, 50], [100, 100], [0, 0], [1, 0]),
        # IoUs exactly on thresholds: 0.5, 0.75 and linspace's own 0.55 .. 0.95
        ([[0.5, 0.75], [float(thr[1]), float(thr[9])], [0.75, 0.5]], [2000, 2000, 2000], [2000, 20], [0, 0], [0, 0]),
        # gt areas on the area-range borders (1024 is inside both small and medium), dets outside the range unmatched -> ignored
        ([[0.7, 0.0, 0.0], [0.0, 0.7, 0.0], [0.0, 0.0, 0.3]], [1024, 9216, 5], [1024, 9216, 10000], [0, 0, 0], [0, 0, 0]),
        ([], [], [10.0, 2000.0], [0, 1], [0, 0]),          # gts, no det
        ([[], []], [10.0, 20000.0], [], [], []),             # dets, no gt
        # ties: equal IoUs take the LATER gt (iou < best skips, equality does not); equal to 1.0 beats min(t, 1 - 1e-10)
        ([[0.8, 0.8, 0.8], [0.8, 0.8, 0.8], [1.0, 1.0, 1.0]], [50, 50, 50], [50, 50, 50], [0, 0, 0], [0, 0, 0]),
    ]
    got = _match_both(ffi, groups, rng, thr)
    assert got[0][0, 0, 0:4].tolist() == [1, 2, 2, 2] and got[1][0, 0, 0:4].tolist() == [0, 1, 1, 1]     # group 0 at t = 0.5, area all
    # group 1 at t = 0.5: det 0 holds gt 1 and never reaches the ignored gt 0 (IoU 0.95); det 1 finds gt 1 taken and takes the ignored gt 0
    assert got[0][0, 0, 4:6].tolist() == [2, 1] and got[1][0, 0, 4:6].tolist() == [0, 1]


def test_coco_match_random_groups(ffi):
    rng = np.random.default_rng(9)
    thr = np.linspace(.5, .95, 10)
    area_rng = [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    groups = []
    for _ in range(300):
        D, G = int(rng.integers(0, 12)), int(rng.integers(0, 8))
        ious = np.round(rng.uniform(0, 1, (D, G)) * 20) / 20 * (rng.uniform(size=(D, G)) < 0.7)       # many ties, many on thresholds
        groups.append((ious.tolist() if G else [[] for _ in range(D)], rng.choice([5.0, 1024.0, 3000.0, 20000.0], D).tolist(),
                       rng.choice([5.0, 1024.0, 3000.0, 9216.0, 20000.0], G).tolist(), (rng.uniform(size=G) < 0.2).astype(int).tolist(),
                       (rng.uniform(size=G) < 0.15).astype(int).tolist()))
    _match_both(ffi, groups, area_rng, thr)
    _match_both(ffi, groups[:40], [[0, 1e10]], [0.5])


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
@pytest.mark.parametrize("use_cats,max_dets", [(1, [1, 10, 100]), (0, [1, 3, 5])])
def test_end_to_end_equals_the_reference(ffi, iou_type, use_cats, max_dets):
    """A few hundred images through COCOeval; maxDets[-1] = 5 with useCats = 0 cuts groups.  Then the same with a memory budget that forces
    chunking: every array identical."""
    from isegmi import cocoeval
    gt, res = data.make_dataset(33, n_images=240)
    runs = []
    for budget in (512 << 20, 1 << 12):
        e = cocoeval.COCOeval(cocoeval.COCOGt(gt), res, iou_type, mem_budget=budget)
        e.params.useCats = use_cats
        e.params.maxDets = list(max_dets)
        e.evaluate(); e.accumulate(); e.summarize()
        runs.append(e)
    e, small = runs
    assert small.timings["chunks"] > 20 and e.timings["chunks"] == 1
    p = e.params
    want = ref.evaluate(gt, res, iou_type, [im["id"] for im in gt["images"]], [c["id"] for c in gt["categories"]], use_cats, sorted(max_dets),
                        p.areaRng, p.iouThrs)
    assert sorted(e.evalImgs) == sorted(want)
    cut = 0
    for key, w in want.items():
        for run in runs:
            g = run.evalImgs[key]
            for name in ("dtScores", "dtMatches", "dtIgnore", "gtMatches", "gtIgnore", "ious"):
                assert np.array_equal(g[name], w[name]), (key, name)
        cut += len(w["dtScores"]) == max_dets[-1]
    assert use_cats or cut > 0
    K = len(gt["categories"]) if use_cats else 1
    pr, rc, sc = ref.accumulate(want, K, sorted(max_dets), len(p.areaRng), p.iouThrs, p.recThrs)
    for run in runs:
        assert np.array_equal(run.eval["precision"], pr) and np.array_equal(run.eval["recall"], rc) and np.array_equal(run.eval["scores"], sc)
        assert np.array_equal(run.stats, ref.summarize(pr, rc, p.iouThrs, sorted(max_dets)))
    assert (e.stats[:3] > 0).all()


def test_engine_results_score_one_against_themselves(ffi):
    """Engine to score: a small Pose2Seg forward through the record loop; its result list (non-empty masks only -- an empty mask has IoU 0 with
    itself and rightly counts as a miss) evaluated against a gt built from those same results: segm AP = 1.  The strings the device RLE emits
    are the strings the evaluator reads."""
    from isegmi import cocoeval
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig, test
    from isegmi.weights import pose2seg_state_dict
    sd = pose2seg_state_dict(1234, width=32, blocks=(1, 1, 1, 1), fpn_channels=32, seg_width=32, seg_blocks=(2, 1))
    rng = np.random.default_rng(17)
    sizes = [(48, 64), (70, 30), (64, 64)]
    imgs = [rng.integers(0, 256, (h, w, 3), np.uint8) for h, w in sizes]
    kps = []
    for n, (h, w) in zip((2, 1, 3), sizes):
        k = np.zeros((n, 17, 3), np.float32)
        k[:, :, 0] = rng.uniform(0.1, 0.9, (n, 17)) * w; k[:, :, 1] = rng.uniform(0.1, 0.9, (n, 17)) * h; k[:, :, 2] = 2
        kps.append(k)
    net = Pose2Seg(sd, Pose2SegConfig(), max_batch=2, max_instances=4)
    results = test(net, imgs, kps, [100, 101, 102])
    net.close()
    results = [r for r in results if coco.rle_area(coco.rle_from_string(r["segmentation"]["counts"])) > 0]
    assert results, "these seeded weights give non-empty masks"
    for k, r in enumerate(results):       # distinct scores: with a tie two identical-score dets may swap gts, which is still AP 1 but not the point
        r["score"] = 1.0 - 1e-3 * k
    gt = {"images": [{"id": 100 + i, "height": h, "width": w} for i, (h, w) in enumerate(sizes)], "categories": [{"id": 1, "name": "person"}],
          "annotations": [{"id": k, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "segmentation": r["segmentation"]}
                          for k, r in enumerate(results)]}
    stats = cocoeval.evaluate_results(gt, results, ("segm", "bbox"))
    assert abs(stats["segm"][0] - 1.0) <= 1e-12 and abs(stats["segm"][1] - 1.0) <= 1e-12 and abs(stats["segm"][8] - 1.0) <= 1e-12
    assert abs(stats["bbox"][0] - 1.0) <= 1e-12


def test_cli_coco_eval(ffi, tmp_path, capsys):
    import json
    from isegmi import cli, cocoeval
    gt, res = data.make_dataset(44, n_images=40)
    (tmp_path / "gt.json").write_text(json.dumps(gt)); (tmp_path / "dt.json").write_text(json.dumps(res))
    out = tmp_path / "stats.json"
    cli.main(["coco_eval", "--gt", str(tmp_path / "gt.json"), "--dt", str(tmp_path / "dt.json"), "--iou-type", "segm", "--max-dets", "1", "10", "100",
              "--out", str(out)])
    e = cocoeval.COCOeval(gt, res, "segm")
    e.evaluate(); e.accumulate()
    lines = e.summarize()
    assert json.loads(out.read_text()) == {"segm": [float(v) for v in e.stats]}
    printed = capsys.readouterr().out
    assert all(l in printed for l in lines)
    only = cocoeval.evaluate_results(gt, res, ("bbox",), cat_ids=[1, 2])["bbox"]
    e = cocoeval.COCOeval(gt, res, "bbox"); e.params.catIds = [1, 2]
    e.evaluate(); e.accumulate(); e.summarize()
    assert np.array_equal(only, e.stats)


@pytest.mark.parametrize("as_string", [False, True])
def test_zero_length_runs_leave_every_number_of_the_evaluation_alone(ffi, as_string):
    """a zero-length run covers no pixel.  Every RLE of a data set -- gts and results -- rewritten with zero-length runs (runs split as
    (a, 0, b), pairs of zeros put in anywhere, the front and the end included), as count lists or as compressed strings: IoUs, matches, areas, precision,
    recall and the twelve numbers are those of the canonical encodings."""
    import copy

    import fuzz_cases as fc
    from isegmi import cocoeval
    gt, res = data.make_dataset(41, n_images=40)
    rng = np.random.default_rng(41)
    gt2, res2 = copy.deepcopy(gt), copy.deepcopy(res)
    n = 0
    for a in gt2["annotations"] + res2:
        seg = a.get("segmentation")
        if isinstance(seg, dict):
            c = seg["counts"]
            z = fc.same_mask_with_zero_runs(rng, coco.rle_from_string(c) if isinstance(c, str) else c)
            assert 0 in z[1:] and np.array_equal(ref.dense(z, *seg["size"]), ref.seg_dense(seg, 0, 0))
            seg["counts"] = coco.rle_to_string(z) if as_string else z
            n += 1
    assert n > 100
    runs = []
    for g, r in ((gt, res), (gt2, res2)):
        e = cocoeval.COCOeval(cocoeval.COCOGt(g), r, "segm")
        e.evaluate(); e.accumulate(); e.summarize()
        runs.append(e)
    plain, zeros = runs
    assert sorted(plain.evalImgs) == sorted(zeros.evalImgs) and len(plain.evalImgs) > 40
    for key, w in plain.evalImgs.items():
        for name in ("dtScores", "dtMatches", "dtIgnore", "gtMatches", "gtIgnore", "ious"):
            assert np.array_equal(zeros.evalImgs[key][name], w[name]), (key, name)
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(zeros.eval[name], plain.eval[name]), name
    assert np.array_equal(zeros.stats, plain.stats) and (plain.stats[:3] > 0).all()
