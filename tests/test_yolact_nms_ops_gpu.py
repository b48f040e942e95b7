"""isegmi_op_yolact_detect in nms_mode 1 (cross-class fast NMS) and 2 (traditional NMS), bit for bit against the restatement in
tests/yolact_nms_ref.py (itself held to a second opinion and to the crafted cases' verdicts by tests/test_yolact_nms_cpu.py)."""
import numpy as np
import pytest

import yolact_nms_ref as R
from oracle import ora

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("prior", "cls", "score", "box", "mask")


def _check(ffi, conf, loc, mask, priors, mode, fused_A=0, cap=1024, **par):
    """one device call against the restatement, image by image; returns (detections, totals, overflow flags) of the restatement"""
    p = dict(conf_thresh=0.05, nms_thr=0.5, top_k=200, max_det=100, max_size=550)
    p.update(par)
    got, boxes, total, over = ffi.yolact_detect(conf, loc, mask, priors, conf_thresh=p["conf_thresh"], nms_thresh=p["nms_thr"], top_k=p["top_k"],
                                                max_det=p["max_det"], nms_mode=mode, trad_cap=cap, max_size=p["max_size"], fused_A=fused_A,
                                                return_nms=True)
    out = []
    for n in range(conf.shape[0]):
        rb = ora.yolact_decode(loc[n], priors)
        assert np.array_equal(boxes[n], rb)
        ref, rt, ro = R.run_ref(mode, ora.softmax(conf[n]), rb, mask[n], p["conf_thresh"], p["nms_thr"], p["top_k"], p["max_det"], p["max_size"], cap)
        assert len(got[n]["score"]) == len(ref["score"]), (n, len(got[n]["score"]), len(ref["score"]))
        for k in KEYS:
            assert np.array_equal(got[n][k], ref[k]), (n, k)
        assert int(total[n]) == rt and int(over[n]) == ro, (n, int(total[n]), rt, int(over[n]), ro)
        out.append((ref, rt, ro))
    return out


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ncls", [2, 5, 81])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 300, 2000])
def test_modes_match_restatement(ffi, P, ncls, mode):
    nd = 0
    for N in (1, 3):
        rng = np.random.default_rng(P * 1000 + ncls * 10 + N)
        conf, loc, mask, priors = R.random_inputs(rng, N, P, ncls=ncls, md=8, hot=0.3)
        if P == 1:
            conf[:, 0, 1] += 9.0   # the one prior is a candidate
        A = 3 if P % 3 == 0 else 1
        for fused in (0, A):   # the three head buffers, then the fused per-pixel row
            res = _check(ffi, conf, loc, mask, priors, mode, fused_A=fused)
            nd += sum(len(r[0]["score"]) for r in res)
    assert nd > 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_empty_image_next_to_full_one(ffi, mode):
    rng = np.random.default_rng(5)
    conf, loc, mask, priors = R.random_inputs(rng, 3, 500, ncls=9, md=8, hot=0.5)
    conf[1, :, 0] += 30.0   # image 1: nothing passes the pre-filter
    if mode == 0:
        got, _, total, over = ffi.yolact_detect(conf, loc, mask, priors, return_nms=True)
        assert [len(g["score"]) > 0 for g in got] == [True, False, True] and total[1] == 0 and not over.any()
        return
    res = _check(ffi, conf, loc, mask, priors, mode)
    assert [r[1] > 0 for r in res] == [True, False, True]


@pytest.mark.parametrize("mode", [1, 2])
def test_all_boxes_identical(ffi, mode):
    rng = np.random.default_rng(6)
    conf, loc, mask, priors = R.random_inputs(rng, 1, 300, ncls=4, md=8, hot=0.8)
    priors[:] = priors[0]
    loc[:] = 0
    res = _check(ffi, conf, loc, mask, priors, mode)
    ncand_classes = ((ora.softmax(conf[0])[:, 1:] > 0.05).sum(0) > 0).sum()
    assert res[0][1] == (1 if mode == 1 else ncand_classes)   # one survivor in all, or one per class that has a candidate


COUNTS = [(m, 1024) for m in (0, 1, 63, 64, 65, 128, 129)] + [(m, 64) for m in (63, 64, 65)] + [(m, 128) for m in (127, 128, 129)] + [(1100, 1024), (2100, 2048)]


@pytest.mark.parametrize("m,cap", COUNTS)
def test_candidate_counts(ffi, m, cap):
    c = R.case_one_class_count(m, extra=7)
    prob = ora.softmax(c["conf"][0])
    assert (prob[:, 1] > 0.05).sum() == m and (prob[:, 2] > 0.05).sum() == 7
    res = _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 2, cap=cap, **c["params"])
    # the flag (already held to the restatement's above): set where the class exceeds a small cap, where fewer than max_det of the visited
    # boxes survive; clear within the cap, and clear at 1100 > 1024 and 2100 > 2048 candidates, where several hundred survive (the last case
    # runs the k > 1024 top-k form and the crowded kernel with more chunks than it has waves)
    assert res[0][2] == (1 if (m, cap) in ((65, 64), (129, 128)) else 0)
    assert m <= 64 or res[0][1] < m   # something was suppressed in the crowded class
    _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 1, **c["params"])


def _crafted():
    return dict(chain=R.case_chain(), two_classes=R.case_two_classes(), edge_plus_one=R.case_edge_plus_one(), edge_plain=R.case_edge_plain(),
                arithmetic=R.case_arithmetic(), class_tie=R.case_class_tie(), at_threshold=R.case_at_threshold(ora.softmax), cut=R.case_cut())


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", sorted(_crafted()))
def test_crafted_cases(ffi, name, mode):
    c = _crafted()[name]
    _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], mode, **c["params"])
    if name == "edge_plain" and mode == 1:   # and one ulp below the threshold the verdict flips on the device as well
        p = dict(c["params"]); p["nms_thr"] = float(np.nextafter(F(p["nms_thr"]), F(0)))
        res = _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 1, **p)
        assert res[0][0]["prior"].tolist() == [0]
    if name == "edge_plus_one" and mode == 2:
        p = dict(c["params"]); p["nms_thr"] = float(np.nextafter(F(0.5), F(1)))
        res = _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 2, **p)
        assert res[0][0]["prior"].tolist() == [0, 1]


@pytest.mark.parametrize("cap", [64, 128])
def test_cap_cases(ffi, cap):
    c = R.case_cap_hidden(cap)
    res = _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 2, cap=cap, **c["params"])
    assert res[0][2] == 1 and res[0][0]["prior"].tolist() == [0]
    c = R.case_cap_harmless(cap, max_det=cap // 2)
    res = _check(ffi, c["conf"], c["loc"], c["mask"], c["priors"], 2, cap=cap, **c["params"])
    assert res[0][2] == 0 and res[0][1] == cap


def test_mode0_through_the_widened_struct(ffi):
    """the appended fields' zero defaults: the default rule against the restatement the existing tests use, with the two new outputs attached"""
    rng = np.random.default_rng(11)
    conf, loc, mask, priors = R.random_inputs(rng, 2, 1500, ncls=81, md=32, hot=0.05)
    got, boxes, total, over = ffi.yolact_detect(conf, loc, mask, priors, return_nms=True)
    plain, _ = ffi.yolact_detect(conf, loc, mask, priors)
    for n in range(2):
        ref = ora.yolact_detect(ora.softmax(conf[n]), ora.yolact_decode(loc[n], priors), mask[n])
        assert len(ref["score"]) > 0
        for k in KEYS:
            assert np.array_equal(got[n][k], ref[k]) and np.array_equal(plain[n][k], ref[k]), k
        assert total[n] >= len(ref["score"]) and over[n] == 0


@pytest.mark.parametrize("kw,name", [(dict(nms_mode=3), "nms_mode"), (dict(nms_mode=2, trad_cap=100), "nms_trad_cap"),
                                     (dict(nms_mode=2, trad_cap=4096), "nms_trad_cap"), (dict(nms_mode=2, trad_cap=32), "nms_trad_cap"),
                                     (dict(nms_mode=1, second_threshold=1), "nms_second_threshold"),
                                     (dict(nms_mode=2, second_threshold=1), "nms_second_threshold")])
def test_refusals_name_the_parameter(ffi, kw, name):
    rng = np.random.default_rng(1)
    conf, loc, mask, priors = R.random_inputs(rng, 1, 64, ncls=3, md=4)
    with pytest.raises(Exception, match=name):
        ffi.yolact_detect(conf, loc, mask, priors, **kw)
