"""The hand-off contract on the CPU: the numpy restatement (tests/pose_handoff_ref.py) on hand-built cases, each of which gives
ANOTHER answer under the wrong rule it is there to catch -- so the GPU tests that run the same cases discriminate --, the pose2seg_test parser and the
scores of results_from_records(kind=3)."""
import numpy as np
import pytest

import pose_handoff_cases as cases
import pose_handoff_ref as ref


def loop_handoff(score, count, kpt, kscore, ratios, person_thresh, kp_thresh, K, *, ge=False, unstable=False, assume_sorted=False, overflow=False,
                 kp_ge=False, no_ratio=False):
    """A second, loop-form statement of the contract with one switch per wrong rule."""
    score = np.asarray(score, np.float32)
    N = score.shape[0]
    pt, kt = np.float32(person_thresh), np.float32(kp_thresh)
    rows, score_out, src_slot, count_out = [], np.zeros((N, K), np.float32), np.full((N, K), -1, np.int32), np.zeros(N, np.int32)
    for n in range(N):
        cand = [j for j in range(int(count[n])) if (score[n, j] >= pt if ge else score[n, j] > pt)]
        if not assume_sorted:   # rank: more candidates beat the later one
            key = (lambda j: (-score[n, j], -j)) if unstable else (lambda j: (-score[n, j], j))
            cand.sort(key=key)
        if len(cand) > K:
            if overflow:
                raise OverflowError("image %d: %d persons" % (n, len(cand)))
            cand = cand[:K]
        count_out[n] = len(cand)
        for r, j in enumerate(cand):
            score_out[n, r], src_slot[n, r] = score[n, j], j
            k = np.empty((17, 3), np.float32)
            rw, rh = (np.float32(1), np.float32(1)) if no_ratio else (np.float32(ratios[n][0]), np.float32(ratios[n][1]))
            k[:, 0] = np.asarray(kpt[n][j], np.float32)[:, 0] * rw
            k[:, 1] = np.asarray(kpt[n][j], np.float32)[:, 1] * rh
            ks = np.asarray(kscore[n][j], np.float32)
            k[:, 2] = np.where(ks >= kt if kp_ge else ks > kt, 2, 0)
            rows.append(k)
    return (np.stack(rows) if rows else np.zeros((0, 17, 3), np.float32)), score_out, src_slot, count_out


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_two_statements_agree_on_every_case():
    for name, c in cases.all_cases().items():
        assert _same(ref.handoff(**c), loop_handoff(**c)), name


def test_strict_person_threshold():
    c = cases.threshold_case()
    got = ref.handoff(**c)
    t = np.float32(c["person_thresh"])
    s = c["score"][0]
    assert s[1] == t and s[0] == np.nextafter(t, np.float32(1)) and s[2] == np.nextafter(t, np.float32(0))
    assert got[3].tolist() == [1] and got[2][0, 0] == 0                   # only the score one ulp above passes
    assert loop_handoff(**c, ge=True)[3].tolist() == [2]                  # >= would keep the one at the threshold too


def test_equal_scores_go_to_the_lower_slot():
    c = cases.ties_case(K=4)
    got = ref.handoff(**c)
    assert not _same(got, loop_handoff(**c, unstable=True))
    blk = got[2][0, :4].tolist()
    assert blk == sorted(blk, key=lambda j: (-c["score"][0, j], j)) and len(set(c["score"][0, blk].tolist())) < 4


def test_tie_block_straddling_the_cut():
    c = cases.ties_case(K=3)
    got = ref.handoff(**c)
    s = c["score"][0]
    kept, cut = got[2][0, :3], [j for j in range(int(c["count"][0])) if s[j] > c["person_thresh"] and j not in got[2][0]]
    assert any(s[j] == s[kept[-1]] and j > kept[-1] for j in cut)          # a slot with the last kept score was cut: the higher slot
    assert not _same(got, loop_handoff(**c, unstable=True))


def test_input_is_ranked_not_assumed_sorted():
    c = cases.ascending_case()
    got = ref.handoff(**c)
    assert (np.diff(c["score"][0, :int(c["count"][0])]) > 0).all()
    assert (np.diff(got[1][0, :int(got[3][0])]) < 0).all()
    assert not _same(got, loop_handoff(**c, assume_sorted=True))


def test_a_surplus_is_cut():
    c = cases.ascending_case()
    assert int((c["score"][0, :int(c["count"][0])] > c["person_thresh"]).sum()) > c["K"]
    got = ref.handoff(**c)
    assert got[3].tolist() == [c["K"]] and len(got[0]) == c["K"]
    with pytest.raises(OverflowError):
        loop_handoff(**c, overflow=True)


def test_keypoint_threshold_is_strict_and_xy_are_copied_either_way():
    c = cases.threshold_case()
    got = ref.handoff(**c)
    ks = c["kscore"][0, 0]
    t = np.float32(c["kp_thresh"])
    assert ks[0] == t and ks[1] == np.nextafter(t, np.float32(3)) and ks[2] == np.nextafter(t, np.float32(0))
    assert got[0][0, :3, 2].tolist() == [0.0, 2.0, 0.0]
    assert loop_handoff(**c, kp_ge=True)[0][0, :3, 2].tolist() == [2.0, 2.0, 0.0]
    assert (got[0][0, :, :2] != 0).all() and set(got[0][0, :, 2].tolist()) == {0.0, 2.0}


def test_ratios_scale_x_and_y_separately():
    c = cases.threshold_case()
    got = ref.handoff(**c)
    rw, rh = np.float32(c["ratios"][0][0]), np.float32(c["ratios"][0][1])
    assert rw != 1 and rh != 1 and rw != rh
    assert np.array_equal(got[0][0, :, 0], c["kpt"][0, 0, :, 0] * rw) and np.array_equal(got[0][0, :, 1], c["kpt"][0, 0, :, 1] * rh)
    assert not _same(got, loop_handoff(**c, no_ratio=True))


def test_slots_beyond_the_count_do_not_leak():
    c = cases.batch_case(K=4)
    assert not np.isfinite(c["score"][1, 5:]).all() and np.isinf(c["score"][0]).any()      # garbage behind the counts (0, 5, 100)
    got = ref.handoff(**c)
    assert got[3][0] == 0 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert (got[2][1, :int(got[3][1])] < 5).all()
    clean = dict(c, score=np.where(np.arange(100)[None] < np.asarray(c["count"])[:, None], c["score"], 0).astype(np.float32))
    assert _same(got, ref.handoff(**clean))


def test_images_pack_in_order_and_empty_batches_give_no_rows():
    c = cases.batch_case(K=128)
    kp, sc, sl, cnt = ref.handoff(**c)
    assert cnt[0] == 0 and 0 < cnt[1] <= 5 and cnt[1] < cnt[2] <= 100 and len(kp) == cnt.sum()
    parts = ref.split(kp, cnt)
    assert [len(p) for p in parts] == cnt.tolist()
    j = sl[2, 0]
    assert np.array_equal(parts[2][0, :, 0], c["kpt"][2, j, :, 0] * np.float32(c["ratios"][2][0]))
    e = cases.empty_case()
    kp, sc, sl, cnt = ref.handoff(**e)
    assert kp.shape == (0, 17, 3) and not cnt.any() and not sc.any() and (sl == -1).all()
    a = cases.all_cut_case()
    kp, sc, sl, cnt = ref.handoff(**a)
    assert cnt.tolist() == [2, 0, 1] and (a["count"] > 0).all()            # image 1 has detections, none above the threshold


def test_cli_parser_takes_the_detector_flags():
    from isegmi import cli
    ap = cli.build_parser()
    a = ap.parse_args(["pose2seg_test", "--anno", "a.json", "--image-root", "d"])
    assert not any(hasattr(a, k) for k in ("keypoint_config", "keypoint_weights", "keypoint_opts", "person_threshold", "keypoint_threshold"))   # nothing changes
    a = ap.parse_args(["pose2seg_test", "--anno", "a.json", "--image-root", "d", "--keypoint-config", "kp.yaml", "--keypoint-weights", "random",
                       "--person-threshold", "0.3", "--gt", "gt.json", "--keypoint-opts", "INPUT.MIN_SIZE_TEST", "192"])
    assert (a.keypoint_config, a.keypoint_weights, a.person_threshold, a.gt) == ("kp.yaml", "random", 0.3, "gt.json")
    assert a.keypoint_opts == ["INPUT.MIN_SIZE_TEST", "192"]
    with pytest.raises(SystemExit, match="--keypoint-config"):
        cli.main(["pose2seg_test", "--anno", "a.json", "--image-root", "d", "--keypoint-weights", "random"])


def test_results_from_records_kind3_scores_come_from_the_record():
    from isegmi.coco import results_from_records
    K = 2
    rec = {"count": np.array([2, 0], np.int32), "box": np.array([[[1, 2, 5, 9], [0, 0, 3, 3]], [[0] * 4] * 2], np.float32),
           "score": np.array([[1.0, 1.0], [0, 0]], np.float32), "label": np.array([[1, 1], [0, 0]], np.int32),
           "str_off": np.array([0, 2, 4, 4, 4], np.int32), "chars": b"abcd"}
    res = results_from_records(rec, [7, 8], [(10, 12), (5, 5)], 3, K)
    assert [(d["image_id"], d["category_id"], d["score"], d["bbox"]) for d in res] == [(7, 1, 1.0, [1.0, 2.0, 4.0, 7.0]), (7, 1, 1.0, [0.0, 0.0, 3.0, 3.0])]
    assert [d["segmentation"] for d in res] == [{"size": [10, 12], "counts": "ab"}, {"size": [10, 12], "counts": "cd"}]
    rec["score"] = np.array([[0.75, 0.5], [0, 0]], np.float32)             # a KeypointPose2Seg step: the detections' box scores
    assert [d["score"] for d in results_from_records(rec, [7, 8], [(10, 12), (5, 5)], 3, K)] == [0.75, 0.5]
