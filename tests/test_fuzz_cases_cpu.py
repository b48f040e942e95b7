"""The generator of the property tests has teeth (tests/fuzz_cases.py; no GPU): for every operator, every profile and seeds 0..7
  (a) the builder's `reached` names the profile's condition, and the condition holds when it is recomputed here from the reference's outputs;
  (b) the reference gives the same bytes twice;
  (c) every wrong-rule switch a reference has changes its answer on at least one (profile, seed) of its operator -- the case is named;
and the references are quick: scaled to the 25 examples a property test draws, the slowest operator's reference time stays under 3 s.
Run with -s to see the table."""
import functools
import time

import numpy as np
import pytest

import bbox_aug_ref
import cocoeval_ref
import fuzz_cases as fc
import keypoint_ref
import pose_handoff_ref
import render_ref
import retinanet_ref
import yolact_nms_ref
import yolov3_ref
from fuzz_cases import bytes_of
from oracle import ora

F = np.float32
SEEDS = range(8)
EXAMPLES, BUDGET_SECONDS = 25, 3.0


@functools.lru_cache(maxsize=None)
def built(op, profile, seed):
    """-> (case, reference answer, reference seconds); built once, shared by the tests, never modified"""
    build, ref, _ = fc.OPS[op]
    case = build(profile, seed)
    t0 = time.perf_counter()
    want = ref(case)
    return case, want, time.perf_counter() - t0


def cases(op):
    return [(p, s) for p in fc.OPS[op][2] for s in SEEDS]


# ------------------------------------------------------------------------------------------------ (a) the conditions, recomputed
def _runs_1(counts, h):
    """[start, end) of the 1-runs of a count list"""
    e = np.cumsum(np.asarray(counts, np.int64)); s = e - np.asarray(counts, np.int64)
    return s[1::2], e[1::2]


def holds_rle_counts(profile, case, want):
    c = [int(v) for v in case["counts"][0]]
    P = case["h"] * case["w"]
    return {"zero_run_first": c[:2] == [0, 0],
            "zero_1run_inside": 0 in c[1:-1:2],                                                   # a zero at an odd index: a 1-run of no pixels
            "zero_0run_inside": any(c[i] == 0 and c[i - 1] > 0 and c[i + 1] > 0 for i in range(2, len(c) - 1, 2)),   # two 1-runs touching
            "zero_run_last": c[-1] == 0,
            "only_zero_runs_then_full": set(c[:-1]) == {0} and c[-1] == P and int(want["area"][0]) in (0, P),
            "more_than_256_runs_with_zeros": len(c) > 256 and 0 in c[1::2] and 0 in c[2::2]}[profile]


def holds_rle_chain(profile, case, want):
    N, K = case["masks"].shape[:2]
    hw, valid, wins, count = case["hw"], case["valid"], case["windows"], case["count"]
    slot = {nk: i for i, nk in enumerate(valid)}
    if profile == "window_on_last_row":
        c0 = int(count[0])
        i = slot[(0, c0 - 1)]
        return c0 < K and tuple(wins[0, c0 - 1, 2:]) == (hw[0, 1], hw[0, 0]) and len(want["counts"][i]) % 2 == 0 and (case["masks"][0, c0] != 0).all()   # an even number of runs: the last pixel is set
    if profile == "window_on_chunk_border":
        return any(wins[n, k, 3] % 64 == 0 and wins[n, k, 3] > 0 and want["bbox"][slot[(n, k)], 3] == wins[n, k, 3] - 1 for n, k in valid)   # the tight box ends on the row before the border
    if profile == "invalid_between_valid":
        flat = [n * K + k for n, k in valid]
        return count is not None and any(m not in flat for m in range(flat[0], flat[-1]))
    if profile == "empty_and_full":
        return any((n, k + 1) in slot and list(want["counts"][i]) == [hw[n].prod()] and list(want["counts"][slot[(n, k + 1)]]) == [0, hw[n].prod()] for (n, k), i in slot.items())
    if profile == "column_wrap":
        for (n, k), i in slot.items():
            s, e = _runs_1(want["counts"][i], hw[n, 0])
            if ((e > s) & (s // hw[n, 0] < (e - 1) // hw[n, 0]) & (s % hw[n, 0] != 0)).any():     # a 1-run that starts inside one column and ends in a later one
                return True
        return False


def holds_pose_handoff(profile, case, want):
    a = case["args"]
    s, c, K, pt = a["score"][0], int(a["count"][0]), a["K"], F(a["person_thresh"])
    order = pose_handoff_ref.select(s, c, pt, len(s))
    if profile == "more_than_K":
        return len(order) > K and want["count"][0] == K
    if profile == "score_tie_at_K":
        return len(order) > K and s[order[K - 1]] == s[order[K]] and order[K - 1] != order[K] and order[K] not in want["slot"][0]
    if profile == "at_person_thresh":
        at = np.flatnonzero(s[:c] == pt)
        return len(at) > 0 and not set(at.tolist()) & set(want["slot"][0].tolist())
    if profile == "none_pass":
        return c > 0 and want["count"][0] == 0 and (want["slot"][0] == -1).all()


def holds_keypoint_decode(profile, case, want):
    heat, boxes, count = case["heat"], case["boxes"], case["count"]
    if profile == "count_zero":
        return count[0] == 0 and count[1:].any() and not want["kpt"][0].any() and not want["kscore"][0].any()
    w, h, wc, hc = keypoint_ref.box_sizes(boxes[0, 0])
    _, score, pos = keypoint_ref.decode_one(heat[0], boxes[0, 0])
    if profile == "argmax_tie":
        r = [keypoint_ref.resize_bicubic(heat[0, :, :, k], hc, wc).reshape(-1) for k in range(heat.shape[3])]
        return all((m == m.max()).sum() >= 2 and int(p) == int(np.flatnonzero(m == m.max())[0]) and s == m.max() for m, p, s in zip(r, pos, want["kscore"][0, 0]))
    if profile == "subpixel_box":
        return (wc, hc) == (1, 1) and w == 1 and h == 1 and (boxes[0, 0, 2] - boxes[0, 0, 0]) < 1 and (pos == 0).all()
    if profile == "huge_box":
        return wc > fc.KEYPOINT_THREADS and hc > 1
    if profile == "peak_on_border":
        axis, last = case["border"]
        line = (pos // wc) if axis == 0 else (pos % wc)
        return (line == ((hc if axis == 0 else wc) - 1 if last else 0)).all()


def _touched(case, entries, dots):
    """pixels an entry / dot list changes: painted over black and over white, one of the two shows every write"""
    H, W = case["image"].shape[:2]
    lo, hi = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    return (render_ref.paint_ref(lo, case["masks"], entries, dots) != lo).any(2) | (render_ref.paint_ref(hi, case["masks"], entries, dots) != hi).any(2)


def holds_paint(profile, case, want):
    H, W = case["image"].shape[:2]
    e, d = case["entries"], case["dots"]
    if profile == "outline_off_image":
        on = e[(e[:, 6] & 1) == 1]
        return (on[:, 1] < 0).any() and (on[:, 2] < 0).any() and (on[:, 3] >= W).any() and (on[:, 4] >= H).any() and ((on[:, 3] < on[:, 1]) | (on[:, 4] < on[:, 2])).any()
    if profile == "dot_off_image":
        off = [k for k in range(len(d)) if not (0 <= d[k, 0] < W and 0 <= d[k, 1] < H)]
        reach = [bool(_touched(case, None, d[k:k + 1]).any()) for k in off]
        return True in reach and False in reach          # off-image centres that still paint, and ones that do not
    if profile == "everything_on_one_pixel":
        both = np.ones((H, W), bool)
        for k in range(len(e)):
            both &= _touched(case, e[k:k + 1], None)
        for k in range(len(d)):
            both &= _touched(case, None, d[k:k + 1])
        return len(e) >= 2 and len(d) >= 2 and both.any()
    if profile == "slot_minus_one_only":
        return len(e) > 0 and np.array_equal(want["image"], render_ref.paint_ref(case["image"], None, e, d))       # the planes are not needed
    if profile == "width_not_multiple_of_4":
        return W % 4 != 0 and want["image"].shape[1] == W


def holds_resample(profile, case, want):
    (h, w), (oh, ow) = case["images"][0].shape[:2], want["views"][0].shape[:2]
    _, _, _, dy, dx, _, _ = case["entries"][0]
    if profile == "one_axis_identity":
        return (oh == h) != (ow == w)
    if profile == "up_one_axis_down_other":
        return (oh > h and ow < w) or (oh < h and ow > w)
    if profile == "rows_cross_chunk":
        return fc.resample_tile_rows(h, oh) > fc.RESAMPLE_CHUNK >= fc.resample_tile_rows(w, ow) or fc.resample_tile_rows(h, oh) > fc.RESAMPLE_CHUNK
    if profile == "image_smaller_than_tile_in_canvas":
        c, fill = want["canvas"][0], F(case["fill"])
        frame = np.ones(c.shape[:2], bool)
        frame[dy:dy + oh, dx:dx + ow] = False
        return oh < 16 and ow < 64 and (c[frame] == fill).all() and frame[0].all() and frame[-1].all() and frame[:, 0].all() and frame[:, -1].all()
    if profile == "one_by_one":
        return (h, w) == (1, 1) or (oh, ow) == (1, 1)


def holds_yolo_select(profile, case, want):
    kw, row = case["kw"], case["heads"][0][0]
    A, top_n, thr, ml = kw["A"], kw["top_n"], kw["thr"], kw["multi_label"]
    C = row.shape[-1] // A - 5
    nrec = row.size // (5 + C)
    with np.errstate(invalid="ignore"):
        sc, idx, total = yolov3_ref.select_level(row, A, 1 << 30, thr, ml)       # every candidate, in order
    assert total == want["total"][0, 0]
    rec = row.reshape(nrec, 5 + C)
    if profile == "slice_border":
        rs = fc.YOLO_SLICE_FLOATS // (5 + C)
        return nrec > rs and {rs - 1, rs} <= set((idx // C).tolist())
    if profile == "tie_at_cut":
        return total > top_n and sc[top_n - 1] == sc[top_n] and idx[top_n - 1] != idx[top_n]
    if profile == "none_pass":
        return total == 0 and all(len(d[0][1]) == 0 for d in want["dec"][:1])
    if profile == "all_pass_over_top_n":
        return total == nrec * (C if ml else 1) > top_n
    if profile == "class_tie_single_label":
        p = yolov3_ref.sigmoid(rec[:, 5:])
        tied = [(r, c) for r, c in zip((idx // C).tolist(), (idx % C).tolist()) if (p[r] == p[r].max()).sum() >= 2]
        return not ml and len(tied) > 0 and all(c == int(np.flatnonzero(p[r] == p[r].max())[0]) for r, c in tied)
    if profile == "nan_inf_box":
        return (~np.isfinite(rec[idx // C, :4]).all(1)).any()
    if profile == "min_wh_edge":
        with np.errstate(invalid="ignore"):
            b = yolov3_ref.decode_level(sc, idx, row, kw["strides"][0], kw["anchors"][0], kw["canvas_w"], kw["canvas_h"], A, 0.0)[0]
            kept = yolov3_ref.decode_level(sc, idx, row, kw["strides"][0], kw["anchors"][0], kw["canvas_w"], kw["canvas_h"], A, kw["min_wh"])[0]
        edge = b[(b[:, 2] - b[:, 0] == F(2)) & (b[:, 3] - b[:, 1] >= F(2))]
        return kw["min_wh"] == 2.0 and len(edge) > 0 and all((kept == e).all(1).any() for e in edge) and len(kept) < len(b)


def holds_retina(profile, case, want):
    row, top_n, thr = case["logits"][0][0], case["top_n"], case["thr"]
    sc, idx = retinanet_ref.select_level(row, 1 << 30, thr)
    if profile == "tie_at_cut":
        return len(sc) > top_n and sc[top_n - 1] == sc[top_n] and idx[top_n - 1] != idx[top_n] and len(want["sel"][0][0][0]) == top_n
    if profile == "at_threshold":
        at = np.flatnonzero(ora.map_f32(row.reshape(-1), 1) == F(thr))
        return len(at) > 0 and not set(at.tolist()) & set(idx.tolist())
    if profile == "empty_level":
        return len(want["sel"][0][0][0]) == 0 and len(want["sel"][-1][0][0]) > 0
    if profile == "cap_cut":
        return want["totals"][0] > case["post"]["det_per_img"]
    if profile == "iou_at_threshold":     # the other comparison at the threshold keeps another set of boxes (seen before the detection cut)
        uncut = dict(case["post"], det_per_img=0, cap=1 << 20)
        return bytes_of(retinanet_ref.postprocess(*want["lists"][0], **dict(uncut, nms_flags=uncut["nms_flags"] ^ 1))) != bytes_of(retinanet_ref.postprocess(*want["lists"][0], **uncut))
    if profile == "all_one_class":
        return len(want["lists"][0][2]) >= 2 and len(set(want["lists"][0][2].tolist())) == 1


def holds_yolact_detect(profile, case, want):
    p = case["params"]
    prob = [ora.softmax(c) for c in case["conf"]]
    boxes = ora.yolact_decode(case["loc"][0], case["priors"])
    fg = prob[0][:, 1:]
    if profile == "empty_next_to_full":
        return any(want[1][n][1] == 0 and len(want[0][n][0]["score"]) == 0 and want[1][n + 1][1] > 0 for n in range(len(prob) - 1))
    if profile == "identical_boxes":
        return want[1][0][1] == 1 and (fg.max(1) > F(0.05)).sum() >= 2          # one box: the cross-class rule keeps one detection
    if profile == "iou_at_threshold":
        ref = lambda mode, thr: yolact_nms_ref.run_ref(mode, prob[0], boxes, case["mask"][0], p["conf_thresh"], thr, p["top_k"], p["max_det"], p["max_size"], p["cap"])   # noqa: E731
        return (bytes_of(ref(1, float(np.nextafter(F(0.5), F(0))))) != bytes_of(want[1][0])            # `<=` at 0.5 keeps what `<` would drop
                and bytes_of(ref(2, float(np.nextafter(F(0.5), F(1))))) != bytes_of(want[2][0]))        # `>=` at 0.5 drops what `>` would keep
    if profile == "class_tie":
        tied = np.flatnonzero((fg.max(1) > F(0.05)) & ((fg == fg.max(1, keepdims=True)).sum(1) >= 2))
        return len(tied) > 0
    if profile == "over_top_k":
        return (fg.max(1) > F(0.05)).sum() > p["top_k"]
    if profile == "over_trad_cap":
        return ((fg > F(0.05)).sum(0) > p["cap"]).any()
    if profile == "P_below_wave":
        return case["conf"].shape[1] < 64


def holds_bbox_aug(profile, case, want):
    v0 = case["views"][0]
    one = lambda v, n, r: len(bbox_aug_ref.candidates(v["logits"][n, r:r + 1], v["regr"][n, r:r + 1], v["props"][n, r:r + 1], 1, v["hw"][n], v["hflip"], v["ratios"],   # noqa: E731
                                                    case["thr"], case["agnostic"])[1])
    if profile == "pool_overflow_mid_row":
        ends = np.cumsum([one(v0, 0, r) for r in range(int(v0["cnt"][0]))])
        return want["pools"][0][1] > case["cap"] == len(want["pools"][0][0][1]) and ends[-1] > case["cap"] and case["cap"] not in ends
    if profile == "zero_proposals":
        return any(v0["cnt"][n] == 0 and want["pools"][n + 1][1] > 0 for n in range(len(v0["cnt"]) - 1))
    if profile == "flip_and_ratio":       # the mirrored view's candidates move when the flip's -1 is dropped, and again when the ratio is
        v = case["views"][-1]
        cand = lambda **kw: bbox_aug_ref.candidates(v["logits"][0], v["regr"][0], v["props"][0], v["cnt"][0], v["hw"][0], kw.get("hflip", v["hflip"]), kw.get("ratios", v["ratios"]),   # noqa: E731
                                                    case["thr"], case["agnostic"], kw.get("wrong"))
        return (len(case["views"]) >= 2 and v["hflip"] and len(cand()[1]) > 0 and bytes_of(cand(wrong="no_minus_one")) != bytes_of(cand())
                and bytes_of(cand(ratios=(1.0, 1.0))) != bytes_of(cand()) and bytes_of(cand(hflip=False)) != bytes_of(cand()))
    if profile == "at_threshold":
        return bytes_of(fc.ref_bbox_aug(case, "ge")["pools"]) != bytes_of(want["pools"])
    if profile == "agnostic":
        return case["agnostic"] and all(v["regr"].shape[-1] == 8 for v in case["views"])


@pytest.mark.parametrize("op", sorted(fc.OPS))
def test_every_profile_reaches_its_condition_for_every_seed(op):
    holds = globals()["holds_" + op]
    for profile in fc.OPS[op][2]:
        hit = []
        for seed in SEEDS:
            case, want, _ = built(op, profile, seed)
            assert profile in case["reached"], (op, profile, seed, sorted(case["reached"]))
            assert holds(profile, case, want), "%s / %s / seed %d: the builder says `reached`, the reference's outputs do not show it" % (op, profile, seed)
            hit.append(seed)
        print("%-16s %-34s reached for seeds %s" % (op, profile, hit))


def test_a_planted_zero_run_is_what_keeps_counts_from_being_canonical():
    """ora.rle_encode(dense(counts)) differs from counts exactly when the list holds a zero behind its first entry"""
    n = 0
    for profile, seed in cases("rle_counts"):
        case = built("rle_counts", profile, seed)[0]
        for k, c in enumerate(case["counts"]):
            again = ora.rle_encode(cocoeval_ref.dense(c, case["h"], case["w"])).tolist()
            planted = 0 in list(c)[1:]
            assert (again != [int(v) for v in c]) == planted, (profile, seed, k, list(c)[:8], again[:8])
            n += planted
        assert all(0 in list(case["counts"][k])[1:] for k in case["planted"]), (profile, seed)
    print("non-canonical count lists:", n)


def test_zero_length_runs_mean_their_dense_decoding_on_the_host():
    """the evaluator accepts any non-negative counts that add up to h * w, as a list or as a compressed string, and a zero-length run
    covers no pixel: area, tight box and the canonical form (rle_merge) are those of the dense decoding.  Negative counts and wrong sums are refused."""
    from isegmi import coco, cocoeval
    seen = 0
    for profile, seed in cases("rle_counts"):
        case = built("rle_counts", profile, seed)[0]
        h, w = case["h"], case["w"]
        for c in case["counts"]:
            c = [int(v) for v in c]
            dense = cocoeval_ref.dense(c, h, w)
            assert cocoeval._seg_counts({"size": [h, w], "counts": c}, None, None) == (c, (h, w))
            s = coco.rle_to_string(c)
            assert coco.rle_from_string(s) == c and cocoeval._seg_counts({"size": [h, w], "counts": s}, None, None) == (c, (h, w)) and s == ora.rle_to_string(c)
            assert coco.rle_area(c) == int(dense.sum()) and coco.rle_to_bbox(c, h) == cocoeval_ref.tight_box(dense)
            assert coco.rle_merge([c], h * w) == coco.rle_counts(dense) and np.array_equal(coco.rle_decode({"size": [h, w], "counts": c}), dense)
            seen += 0 in c[1:]
        rng = np.random.default_rng(seed)
        for c in case["counts"]:
            z = fc.same_mask_with_zero_runs(rng, c)
            assert 0 in z[1:] and np.array_equal(cocoeval_ref.dense(z, h, w), cocoeval_ref.dense(c, h, w))
    assert seen > 100
    for bad in ([5, -1, 2], [3, 4], [0, 0, 5]):
        with pytest.raises(ValueError, match="do not add up"):
            cocoeval._seg_counts({"size": [2, 3], "counts": bad}, None, None)
    gt = cocoeval.COCOGt({"images": [{"id": 1, "height": 3, "width": 4}], "categories": [{"id": 1}],
                          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "segmentation": {"size": [3, 4], "counts": [0, 0, 4, 0, 0, 2, 6, 0, 0]}}]})
    assert gt.anns[0]["area"] == 2.0 and gt.anns[0]["bbox"] == [1.0, 1.0, 1.0, 2.0]       # pixels 4 and 5, column-major in a height of 3: column 1, rows 1..2


# ------------------------------------------------------------------------------------------------ (b) determinism
@pytest.mark.parametrize("op", sorted(fc.OPS))
def test_builder_and_reference_give_the_same_bytes_twice(op):
    build, ref, profiles = fc.OPS[op]
    for profile, seed in cases(op):
        case, want, _ = built(op, profile, seed)
        again = build(profile, seed)
        assert bytes_of({k: v for k, v in again.items() if k != "reached"}) == bytes_of({k: v for k, v in case.items() if k != "reached"}) and again["reached"] == case["reached"]
        assert bytes_of(ref(case)) == bytes_of(want), (op, profile, seed)


# ------------------------------------------------------------------------------------------------ (c) the wrong rules
WRONG = [("yolo_select", dict(ge_threshold=True)), ("yolo_select", dict(tie_high_index=True)), ("yolo_select", dict(best_by_logit=True)), ("yolo_select", dict(swap_xy=True)),
         ("retina", dict(ge_threshold=True)), ("retina", dict(tie_high_index=True)),
         ("bbox_aug", dict(wrong="no_minus_one")), ("bbox_aug", dict(wrong="clip_last")), ("bbox_aug", dict(wrong="ge"))]


@pytest.mark.parametrize("op,fork", WRONG, ids=lambda v: v if isinstance(v, str) else "-".join("%s" % x for x in v.values()))
def test_wrong_rules_are_told_apart(op, fork):
    ref = fc.OPS[op][1]
    apart = []
    for profile, seed in cases(op):
        case, want, _ = built(op, profile, seed)
        with np.errstate(invalid="ignore"):
            if bytes_of(ref(case, **fork)) != bytes_of(want):
                apart.append("%s/%d" % (profile, seed))
    print("%-12s %-28s told apart on %d of %d cases, first %s" % (op, fork, len(apart), len(cases(op)), apart[:3]))
    assert apart, "no (profile, seed) of %s separates %s from the right rule" % (op, fork)


def test_flip_before_clip_is_the_switch_that_changes_nothing():
    """tests/bbox_aug_ref.py says so of its own switch (the mirror maps the clip range onto itself): the generated cases agree"""
    for profile, seed in cases("bbox_aug"):
        case, want, _ = built("bbox_aug", profile, seed)
        assert bytes_of(fc.ref_bbox_aug(case, "flip_before_clip")) == bytes_of(want), (profile, seed)


# ------------------------------------------------------------------------------------------------ the references are quick
def test_reference_time_of_25_examples_stays_under_three_seconds():
    worst = 0.0
    for op in sorted(fc.OPS):
        t = [built(op, p, s)[2] for p, s in cases(op)]
        per25 = EXAMPLES * float(np.mean(t))
        worst = max(worst, per25)
        print("%-16s reference: mean %.2f ms, max %.2f ms a case, %.3f s for %d examples" % (op, 1e3 * np.mean(t), 1e3 * np.max(t), per25, EXAMPLES))
    assert worst < BUDGET_SECONDS, worst
