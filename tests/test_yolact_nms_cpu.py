"""Yolact's cross-class fast NMS and traditional NMS on the CPU: the restatement (tests/yolact_nms_ref.py) against a second opinion written
independently of it, the crafted cases proved to discriminate, the cap lemma by brute force, and config / CLI / refusals."""
import warnings

import numpy as np
import pytest
import torch

import yolact_nms_ref as R
from oracle import ora

F = np.float32


# ------------------------------------------------------------------------------------------------ second opinion
def _jaccard_torch(a, b):
    """box_utils.jaccard / intersect for one batch, as upstream writes it"""
    A, B = a.size(0), b.size(0)
    max_xy = torch.min(a[:, 2:].unsqueeze(1).expand(A, B, 2), b[:, 2:].unsqueeze(0).expand(A, B, 2))
    min_xy = torch.max(a[:, :2].unsqueeze(1).expand(A, B, 2), b[:, :2].unsqueeze(0).expand(A, B, 2))
    inter = torch.clamp(max_xy - min_xy, min=0)
    inter = inter[:, :, 0] * inter[:, :, 1]
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).unsqueeze(1).expand_as(inter)
    area_b = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).unsqueeze(0).expand_as(inter)
    return inter / (area_a + area_b - inter)


def _cc_fast_nms_torch(prob, boxes, conf_thresh, thr, top_k):
    """Detect.detect's pre-filter + cc_fast_nms, line by line (scores [classes, priors])"""
    cur = torch.from_numpy(prob[:, 1:].T.copy())
    conf_scores, _ = torch.max(cur, dim=0)
    keep = conf_scores > conf_thresh
    scores = cur[:, keep]
    b = torch.from_numpy(boxes)[keep, :]
    orig = torch.arange(prob.shape[0])[keep]
    if scores.size(1) == 0:
        return np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, np.int64)
    scores, classes = scores.max(dim=0)
    _, idx = scores.sort(0, descending=True)
    idx = idx[:top_k]
    boxes_idx = b[idx]
    iou = _jaccard_torch(boxes_idx, boxes_idx)
    iou.triu_(diagonal=1)
    iou_max, _ = torch.max(iou, dim=0)
    idx_out = idx[iou_max <= thr]
    return orig[idx_out].numpy(), scores[idx_out].numpy(), classes[idx_out].numpy()


def _cnms_loop(dets, thresh):
    """utils/cython_nms.pyx, a literal loop port in fp32 scalars"""
    x1, y1, x2, y2, scores = (dets[:, i] for i in range(5))
    areas = (x2 - x1 + F(1)) * (y2 - y1 + F(1))
    order = scores.argsort()[::-1]
    ndets = dets.shape[0]
    suppressed = np.zeros(ndets, np.int64)
    keep = []
    for _i in range(ndets):
        i = order[_i]
        if suppressed[i] == 1:
            continue
        keep.append(i)
        ix1, iy1, ix2, iy2, iarea = x1[i], y1[i], x2[i], y2[i], areas[i]
        for _j in range(_i + 1, ndets):
            j = order[_j]
            if suppressed[j] == 1:
                continue
            xx1 = max(ix1, x1[j]); yy1 = max(iy1, y1[j]); xx2 = min(ix2, x2[j]); yy2 = min(iy2, y2[j])
            w = max(F(0.0), F(xx2 - xx1 + F(1))); h = max(F(0.0), F(yy2 - yy1 + F(1)))
            inter = F(w * h)
            ovr = F(inter / F(F(iarea + areas[j]) - inter))
            if ovr >= thresh:
                suppressed[j] = 1
    return keep


def _traditional_nms_torch(prob, boxes, conf_thresh, thr, max_det, max_size):
    """Detect.detect's pre-filter + traditional_nms, as upstream writes it (numpy where upstream leaves torch)"""
    cur = prob[:, 1:].T
    keep = cur.max(0) > F(conf_thresh)
    scores = cur[:, keep]
    orig = np.arange(prob.shape[0])[keep]
    b = (boxes[keep] * F(max_size)).astype(F)
    idx_lst, cls_lst, scr_lst = [], [], []
    for _cls in range(scores.shape[0]):
        cls_scores = scores[_cls, :]
        conf_mask = cls_scores > F(conf_thresh)
        idx = np.arange(cls_scores.shape[0])
        cls_scores = cls_scores[conf_mask]
        idx = idx[conf_mask]
        if cls_scores.shape[0] == 0:
            continue
        preds = np.concatenate([b[conf_mask], cls_scores[:, None]], 1).astype(F)
        k = np.asarray(_cnms_loop(preds, F(thr)), np.int64)
        idx_lst.append(idx[k]); cls_lst.append(k * 0 + _cls); scr_lst.append(cls_scores[k])
    if not idx_lst:
        return np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, np.int64), 0
    idx = np.concatenate(idx_lst); classes = np.concatenate(cls_lst); scores = np.concatenate(scr_lst)
    s, idx2 = torch.from_numpy(scores).sort(0, descending=True)
    idx2 = idx2[:max_det].numpy()
    return orig[idx[idx2]], s[:max_det].numpy(), classes[idx2], len(idx)


def _problem(seed, P=160, ncls=7):
    rng = np.random.default_rng(seed)
    conf, loc, mask, priors = R.random_inputs(rng, 1, P, ncls=ncls, md=4, hot=0.5)
    prob = ora.softmax(conf[0])
    boxes = ora.yolact_decode(loc[0], priors)
    fg = prob[:, 1:]
    assert len(np.unique(fg)) == fg.size, "exact score ties: torch's order is unspecified there"
    return prob, boxes, mask[0]


@pytest.mark.parametrize("seed", range(6))
def test_cc_fast_nms_against_torch(seed):
    prob, boxes, mask = _problem(seed)
    for top_k in (200, 40):
        ref, total = R.cc_fast_nms(prob, boxes, mask, 0.05, 0.5, top_k, 300)
        idx, score, cls = _cc_fast_nms_torch(prob, boxes, 0.05, 0.5, top_k)
        assert total == len(idx) > 3 and total < min(top_k, (prob[:, 1:].max(1) > 0.05).sum()), "nothing suppressed"
        assert np.array_equal(ref["prior"], idx) and np.array_equal(ref["score"], score) and np.array_equal(ref["cls"], cls)
        cut, total2 = R.cc_fast_nms(prob, boxes, mask, 0.05, 0.5, top_k, 3)
        assert total2 == total and np.array_equal(cut["prior"], idx[:3])


@pytest.mark.parametrize("seed", range(6))
def test_traditional_nms_against_loop_port(seed):
    prob, boxes, mask = _problem(seed)
    for max_det in (300, 5):
        ref, total, over = R.traditional_nms(prob, boxes, mask, 0.05, 0.5, max_det, 550)
        idx, score, cls, t2 = _traditional_nms_torch(prob, boxes, 0.05, 0.5, max_det, 550)
        assert over == 0 and total == t2 > 3
        assert total < (prob[:, 1:] > 0.05).sum(), "nothing suppressed"
        assert np.array_equal(ref["prior"], idx) and np.array_equal(ref["score"], score) and np.array_equal(ref["cls"], cls)
        assert np.array_equal(ref["box"], boxes[idx]) and np.array_equal(ref["mask"], mask[idx])


# ------------------------------------------------------------------------------------------------ crafted cases
def _run(case, mode, **over):
    p = dict(case["params"]); p.update(over)
    prob = ora.softmax(case["conf"][0])
    boxes = ora.yolact_decode(case["loc"][0], case["priors"])
    if mode == 0:
        d = ora.yolact_detect(prob, boxes, case["mask"][0], p["conf_thresh"], p["nms_thr"], p["top_k"], p["max_det"])
        return d, None, 0
    return R.run_ref(mode, prob, boxes, case["mask"][0], p["conf_thresh"], p["nms_thr"], p["top_k"], p["max_det"], p["max_size"], p.get("cap"))


def _second(case, mode, **over):
    p = dict(case["params"]); p.update(over)
    prob = ora.softmax(case["conf"][0])
    boxes = ora.yolact_decode(case["loc"][0], case["priors"])
    if mode == 1:
        return _cc_fast_nms_torch(prob, boxes, p["conf_thresh"], p["nms_thr"], p["top_k"])[0][:p["max_det"]]
    return _traditional_nms_torch(prob, boxes, p["conf_thresh"], p["nms_thr"], p["max_det"], p["max_size"])[0]


def _pc(d):
    """(prior, class) pairs: the default rule ranks a kept prior in EVERY class, so its lists also hold the priors' near-zero other classes"""
    return set(zip(d["prior"].tolist(), d["cls"].tolist()))


def test_case_boxes_decode_exactly():
    c = R.case_edge_plus_one()
    boxes = ora.yolact_decode(c["loc"][0], c["priors"]) * F(R.CASE_MAX_SIZE)
    assert np.array_equal(boxes, np.asarray([[64, 64, 67, 67], [64, 64, 67, 65]], F))


def test_chain_greedy_keeps_what_fast_drops():
    c = R.case_chain()
    assert {(0, 1)} <= _pc(_run(c, 0)[0]) and not {(1, 1), (2, 1)} & _pc(_run(c, 0)[0])
    assert _run(c, 1)[0]["prior"].tolist() == [0]
    assert _run(c, 2)[0]["prior"].tolist() == [0, 2] == _second(c, 2).tolist()


def test_two_classes_cross_class_keeps_one():
    c = R.case_two_classes()
    assert {(0, 0), (1, 2)} <= _pc(_run(c, 0)[0]) and _run(c, 2)[0]["prior"].tolist() == [0, 1]
    d, total, _ = _run(c, 1)
    assert d["prior"].tolist() == [0] == _second(c, 1).tolist() and d["cls"].tolist() == [0] and total == 1


def test_plus_one_edge_is_ge():
    c = R.case_edge_plus_one()
    b = ora.yolact_decode(c["loc"][0], c["priors"]) * F(R.CASE_MAX_SIZE)
    assert R.cnms_keep(b, 0.5).tolist() == [0]                             # ovr == thr: suppressed
    assert R.cnms_keep(b, np.nextafter(F(0.5), F(1))).tolist() == [0, 1]   # the next threshold up: kept, so `>` would have kept it at 0.5
    assert _run(c, 2)[0]["prior"].tolist() == [0] == _second(c, 2).tolist()
    assert _run(c, 1)[0]["prior"].tolist() == [0, 1]                        # plain IoU 1/3


def test_plain_edge_is_le():
    c = R.case_edge_plain()
    thr = F(c["params"]["nms_thr"])
    b = ora.yolact_decode(c["loc"][0], c["priors"])
    assert R.jaccard(b)[0, 1] == thr
    assert _run(c, 1)[0]["prior"].tolist() == [0, 1] == _second(c, 1).tolist()
    assert _run(c, 1, nms_thr=float(np.nextafter(thr, F(0))))[0]["prior"].tolist() == [0]   # `<` would have dropped it


def test_arithmetics_disagree():
    c = R.case_arithmetic()
    assert _run(c, 1)[0]["prior"].tolist() == [0, 1] == _second(c, 1).tolist()
    assert _run(c, 2)[0]["prior"].tolist() == [0] == _second(c, 2).tolist()


def test_class_tie_goes_to_the_lowest_class():
    c = R.case_class_tie()
    prob = ora.softmax(c["conf"][0])
    assert prob[0, 2] == prob[0, 4] == prob[0, 1:].max()
    d = _run(c, 1)[0]
    assert d["prior"].tolist() == [0, 1] and d["cls"].tolist() == [1, 2]
    assert sorted(_run(c, 2)[0]["cls"].tolist()) == [1, 2, 3]             # per class the prior is a candidate of both


def test_score_at_threshold_is_no_candidate():
    c = R.case_at_threshold(ora.softmax)
    d2 = _run(c, 2)[0]
    assert 3 not in d2["cls"].tolist() and d2["prior"].tolist() == [1, 0] == _second(c, 2).tolist()
    d0 = _run(c, 0)[0]
    assert 3 in d0["cls"].tolist()                                          # the default rule ranks the prior in class 4 (0-based 3) as well
    lower = float(np.nextafter(F(c["params"]["conf_thresh"]), F(0)))
    assert 3 in _run(c, 2, conf_thresh=lower)[0]["cls"].tolist()            # one ulp lower and it is a candidate


@pytest.mark.parametrize("mode", [1, 2])
def test_cut_and_total(mode):
    c = R.case_cut()
    d, total, _ = _run(c, mode)
    assert total == 30 and len(d["score"]) == 20
    full = _run(c, mode, max_det=100)[0]
    assert len(full["score"]) == 30 and np.array_equal(full["prior"][:20], d["prior"])
    assert np.array_equal(d["prior"], _second(c, mode))


# ------------------------------------------------------------------------------------------------ the cap lemma
def test_cap_lemma_brute_force():
    seen_clear_over_cap = 0
    for seed in range(40):
        rng = np.random.default_rng(500 + seed)
        P = int(rng.integers(100, 400))
        conf, loc, mask, priors = R.random_inputs(rng, 1, P, ncls=4, md=2, hot=0.9)
        prob = ora.softmax(conf[0]); boxes = ora.yolact_decode(loc[0], priors)
        for cap in (64, 128):
            for max_det in (5, 40, 100):
                full, tf, _ = R.traditional_nms(prob, boxes, mask[0], 0.05, 0.5, max_det, 550)
                cut, tc, over = R.traditional_nms(prob, boxes, mask[0], 0.05, 0.5, max_det, 550, cap=cap)
                over_cap = ((prob[:, 1:] > 0.05).sum(0) > cap).any()
                if not over:
                    assert R.same(full, cut), (seed, cap, max_det)
                    seen_clear_over_cap += bool(over_cap)
                else:
                    assert over_cap
    assert seen_clear_over_cap > 0


@pytest.mark.parametrize("cap", [64, 128])
def test_cap_lemma_constructed(cap):
    c = R.case_cap_hidden(cap)
    full = _run(c, 2)[0]
    cut, _, over = _run(c, 2, cap=cap)
    assert over == 1 and full["prior"].tolist() == [0, cap] and cut["prior"].tolist() == [0]
    c = R.case_cap_harmless(cap, max_det=cap // 2)
    full, tf, _ = _run(c, 2)
    cut, tc, over = _run(c, 2, cap=cap)
    assert over == 0 and R.same(full, cut) and tf == cap + 1 and tc == cap and len(cut["score"]) == cap // 2


# ------------------------------------------------------------------------------------------------ config, CLI, refusals
def test_config_maps_the_booleans_as_upstream():
    from isegmi.yolact import YolactConfig, nms_mode_of
    assert YolactConfig().nms_mode == 0 and YolactConfig().use_fast_nms is True and YolactConfig().use_cross_class_nms is False
    assert YolactConfig().nms_trad_cap == 1024
    assert YolactConfig(use_cross_class_nms=True).nms_mode == 1
    assert YolactConfig(use_fast_nms=False).nms_mode == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert nms_mode_of(True, False) == 0 and nms_mode_of(True, True) == 1 and nms_mode_of(False, False) == 2
    with pytest.warns(UserWarning, match="cross-class traditional NMS"):
        assert nms_mode_of(False, True) == 2
    assert YolactConfig(use_fast_nms=False, use_cross_class_nms=True).nms_mode == 2
    for make in (YolactConfig.base, YolactConfig.plus_base, YolactConfig.plus_resnet50, YolactConfig.im700, YolactConfig.darknet53):
        assert make().nms_mode == 0 and make().nms_trad_cap == 1024


@pytest.mark.parametrize("cap", [0, 32, 63, 65, 100, 2112, 4096, -64, 1024.0, True])
def test_config_refuses_cap_by_name(cap):
    from isegmi.yolact import YolactConfig
    with pytest.raises(ValueError, match="nms_trad_cap"):
        YolactConfig(use_fast_nms=False, nms_trad_cap=cap)


@pytest.mark.parametrize("cap", [64, 128, 1024, 1984, 2048])
def test_config_accepts_cap(cap):
    from isegmi.yolact import YolactConfig
    assert YolactConfig(nms_trad_cap=cap).nms_trad_cap == cap


@pytest.mark.parametrize("kw", [dict(use_cross_class_nms=True), dict(use_fast_nms=False)])
def test_config_refuses_second_threshold_by_name(kw):
    from isegmi.yolact import YolactConfig
    with pytest.raises(ValueError, match="nms_second_threshold"):
        YolactConfig(nms_second_threshold=1, **kw)
    assert YolactConfig(nms_second_threshold=1).nms_mode == 0


def test_config_refuses_non_bool():
    from isegmi.yolact import YolactConfig
    with pytest.raises(TypeError, match="use_fast_nms"):
        YolactConfig(use_fast_nms="False")


def test_cli_arguments():
    from isegmi.cli import build_parser, eval_nms_options
    from isegmi.yolact import YolactConfig
    import dataclasses
    d = eval_nms_options(build_parser().parse_args(["eval"]))
    assert d == dict(use_fast_nms=True, use_cross_class_nms=False, nms_trad_cap=1024)
    assert dataclasses.replace(YolactConfig.base(), **d) == YolactConfig.base()
    d = eval_nms_options(build_parser().parse_args(["eval", "--fast_nms", "False", "--cross_class_nms=True", "--nms_trad_cap", "128"]))
    assert d == dict(use_fast_nms=False, use_cross_class_nms=True, nms_trad_cap=128)
    assert eval_nms_options(build_parser().parse_args(["eval", "--fast_nms=true", "--cross_class_nms", "yes"]))["use_cross_class_nms"] is True
    with pytest.raises(SystemExit):
        build_parser().parse_args(["eval", "--fast_nms", "maybe"])
