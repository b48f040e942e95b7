"""Property tests (hypothesis) of the detection tails, the encoders, the painter and the resampler on the cases of tests/fuzz_cases.py: each test draws a
(profile, seed), builds the case -- which CONSTRUCTS the profile's condition, asserted here through `reached` -- runs the `_ffi` wrapper and compares
with the numpy / oracle restatement.  Every comparison is exact: lists and counts with np.array_equal, floats by bit pattern, bytes as bytes, IoUs as
float64 equality.  Outputs the wrappers poison must stay poisoned where the contract says nothing is written.  Each test runs its first example twice
and wants identical bytes.  Derandomised and without a database: a run is reproducible and writes nothing into the tree.
ISEGMI_FUZZ_SCALE=20 lengthens the sweep, as for tests/test_fuzz_gpu.py.

Per-test wall time on an MI355X at the default 25 examples (pytest --durations, one run; reference and builder time included):
    rle_iou_on_hand_written_counts 0.25 s   rle_encode_then_iou 0.07 s   pose_handoff 0.02 s   keypoint_decode 0.04 s   paint 0.05 s
    resample_u8_both_epilogues 0.11 s   yolo_select 0.05 s   retina_select_decode_postprocess 0.23 s   yolact_detect 0.06 s   bbox_aug 0.08 s
The whole module: 1.4 s.
"""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import fuzz_cases as fc
from fuzz_cases import bytes_of
from conv_ref import same_bits

pytestmark = pytest.mark.gpu
_X = int(os.environ.get("ISEGMI_FUZZ_SCALE", "1"))
SET = dict(max_examples=25 * _X, deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
SEED = st.integers(0, 2 ** 31 - 1)
_twice = set()


def once_again(name, run, got):
    """the first example of a test runs a second time: identical bytes"""
    if name not in _twice:
        _twice.add(name)
        assert bytes_of(run()) == bytes_of(got), name + ": two runs of one case differ"


def case_of(op, profile, seed):
    build, ref, profiles = fc.OPS[op]
    case = build(profile, seed)
    assert profile in case["reached"], (op, profile, seed, case["reached"])
    return case, ref(case)


# ---------------------------------------------------------------------------------------------------------------- RLE
def run_rle_counts(ffi, case):
    M = len(case["counts"])
    rles = ffi.RleSet(case["counts"], [(case["h"], case["w"])] * M)
    try:
        return dict(area=rles.area.copy(), bbox=rles.bbox.copy(), iou=ffi.rle_iou(rles, case["pairs"]))
    finally:
        rles.free()


@settings(**SET)
@given(profile=st.sampled_from(fc.RLE_COUNTS_PROFILES), seed=SEED)
def test_rle_iou_on_hand_written_counts_with_zero_runs(ffi, profile, seed):
    """Count lists no encoder would write -- zero-length runs in front, inside (of either parity), at the end, nothing but zero runs before one full
    run, zeros on the seam of the prefix scan's 256-run rounds -- mean what their dense decoding means: area, tight box and IoU."""
    case, want = case_of("rle_counts", profile, seed)
    got = run_rle_counts(ffi, case)
    assert np.array_equal(got["area"], want["area"]), (profile, seed, got["area"], want["area"])
    assert np.array_equal(got["bbox"], want["bbox"]), (profile, seed, got["bbox"].tolist(), want["bbox"].tolist())
    assert got["iou"].dtype == np.float64 and np.array_equal(got["iou"], want["iou"]), (profile, seed, np.flatnonzero(got["iou"] != want["iou"]).tolist())
    M = len(case["counts"])
    assert np.array_equal(got["iou"][:M], (want["area"] > 0).astype(np.float64))               # with itself: 1.0, or 0.0 when empty
    assert not got["iou"][M:M + 2].any()                                                      # with its complement: 0.0, crowd or not
    assert np.array_equal(got["iou"][M + 2:M + 4], np.full(2, float(want["area"][0] > 0)))    # with its canonical twin: the same mask
    once_again("rle_counts", lambda: run_rle_counts(ffi, case), got)


def run_rle_chain(ffi, case):
    """rle_encode, then the counts it produced on the device -- and a complement of each, a zero-length 0-run in front -- straight into RleSet"""
    ro, cn, so, ch, st_ = ffi.rle_encode(case["masks"], case["count"], case["image_hw"], windows=case["windows"])
    K = case["masks"].shape[1]
    lists = [cn[ro[n * K + k]:ro[n * K + k + 1]] for n, k in case["valid"]]
    V = len(lists)
    hw = [case["hw"][n] for n, k in case["valid"]]
    out = dict(run_off=ro, counts=cn[:ro[-1]], str_off=so, chars=ch[:so[-1]], status=st_)
    if all(len(c) for c in lists):      # (an encoder that dropped a slot fails on run_off below; RleSet is not asked to take the wreck)
        rles = ffi.RleSet(lists + [np.concatenate([[0], c]) for c in lists], hw + hw)
        try:
            pairs = np.concatenate([[(i, i, 0) for i in range(V)], [(i, V + i, i & 1) for i in range(V)], case["pairs"]]).astype(np.int32)
            out.update(area=rles.area.copy(), bbox=rles.bbox.copy(), iou=ffi.rle_iou(rles, pairs))
        finally:
            rles.free()
    return out


@settings(**SET)
@given(profile=st.sampled_from(fc.RLE_CHAIN_PROFILES), seed=SEED)
def test_rle_encode_then_iou_on_the_device_counts(ffi, profile, seed):
    """Encoder output -> IoU with no host re-encoding in between: counts and strings equal the oracle's for every valid slot, invalid slots hold no
    runs, garbage outside the windows and in invalid slots is never read; then area, tight box and IoU of the device's own counts."""
    case, want = case_of("rle_chain", profile, seed)
    got = run_rle_chain(ffi, case)
    N, K = case["masks"].shape[:2]
    ro, so = got["run_off"], got["str_off"]
    assert got["status"][2] == 0, "overflow flagged"
    slot = {nk: i for i, nk in enumerate(case["valid"])}
    for n in range(N):
        for k in range(K):
            m = n * K + k
            if (n, k) not in slot:
                assert ro[m + 1] == ro[m] and so[m + 1] == so[m], (profile, seed, n, k)
                continue
            i = slot[(n, k)]
            assert np.array_equal(got["counts"][ro[m]:ro[m + 1]], want["counts"][i]), (profile, seed, n, k, got["counts"][ro[m]:ro[m + 1]][:8], want["counts"][i][:8])
            assert got["chars"][so[m]:so[m + 1]] == want["strings"][i].encode("ascii"), (profile, seed, n, k)
    assert ro[0] == 0 and so[0] == 0 and got["status"][0] == ro[-1] == sum(len(c) for c in want["counts"]) and got["status"][1] == so[-1] == sum(len(s) for s in want["strings"])
    V = len(case["valid"])
    P = case["hw"][[n for n, k in case["valid"]]].prod(1)
    assert np.array_equal(got["area"], np.concatenate([want["area"], P - want["area"]]))
    assert np.array_equal(got["bbox"][:V], want["bbox"])
    iou = got["iou"]
    assert np.array_equal(iou[:V], (want["area"] > 0).astype(np.float64))      # with itself
    assert not iou[V:2 * V].any()                                              # with its complement
    assert np.array_equal(iou[2 * V:], want["iou"]), (profile, seed)
    once_again("rle_chain", lambda: run_rle_chain(ffi, case), got)


# ---------------------------------------------------------------------------------------------------------------- keypoints
def run_pose_handoff(ffi, case):
    a = case["args"]
    kp, sc, sl, cnt = ffi.pose_handoff(a["score"], a["count"], a["kpt"], a["kscore"], a["ratios"], a["person_thresh"], a["kp_thresh"], a["K"])
    return dict(kpts=kp, score=sc, slot=sl, count=cnt)


@settings(**SET)
@given(profile=st.sampled_from(fc.POSE_HANDOFF_PROFILES), seed=SEED)
def test_pose_handoff(ffi, profile, seed):
    case, want = case_of("pose_handoff", profile, seed)
    got = run_pose_handoff(ffi, case)
    R = int(want["count"].sum())
    N, K = case["args"]["score"].shape[0], case["args"]["K"]
    assert np.array_equal(got["count"], want["count"]), (profile, seed)
    assert same_bits(got["score"], want["score"]) and np.array_equal(got["slot"], want["slot"]), (profile, seed)
    assert got["kpts"].shape == (N * K, 17, 3) and same_bits(got["kpts"][:R], want["kpts"]), (profile, seed)
    assert (got["kpts"][R:].view(np.uint8) == 0xFF).all(), "rows behind the last person were written"
    assert np.isfinite(got["kpts"][:R]).all() and np.isfinite(got["score"]).all()      # nothing of the NaN behind the counts came through
    once_again("pose_handoff", lambda: run_pose_handoff(ffi, case), got)


def run_keypoint_decode(ffi, case):
    kpt, ks = ffi.keypoint_decode(case["heat"], case["boxes"], case["count"])
    return dict(kpt=kpt, kscore=ks)


@settings(**SET)
@given(profile=st.sampled_from(fc.KEYPOINT_PROFILES), seed=SEED)
def test_keypoint_decode(ffi, profile, seed):
    case, want = case_of("keypoint_decode", profile, seed)
    got = run_keypoint_decode(ffi, case)
    assert same_bits(got["kpt"], want["kpt"]) and same_bits(got["kscore"], want["kscore"]), (profile, seed, np.argwhere(got["kpt"] != want["kpt"])[:4].tolist())
    for n, c in enumerate(case["count"]):      # slots at or beyond count: zeros over the wrapper's poison, whatever their (NaN) maps hold
        assert not got["kpt"][n, c:].view(np.uint32).any() and not got["kscore"][n, c:].view(np.uint32).any(), (profile, seed, n)
    once_again("keypoint_decode", lambda: run_keypoint_decode(ffi, case), got)


# ---------------------------------------------------------------------------------------------------------------- painter, resampler
PAINT_TAIL, PAINT_SENTINEL = 64, 0xA5


def run_paint(ffi, case, inplace, offset):
    rc, out, src = ffi.paint(case["image"], case["masks"], case["entries"], case["dots"], inplace=inplace, tail=PAINT_TAIL, sentinel=PAINT_SENTINEL, offset=offset)
    return dict(rc=np.int64(rc), out=out, src=src)


@settings(**SET)
@given(profile=st.sampled_from(fc.PAINT_PROFILES), seed=SEED, inplace=st.booleans(), offset=st.sampled_from([0, 1, 2, 3]))
def test_paint(ffi, profile, seed, inplace, offset):
    case, want = case_of("paint", profile, seed)
    got = run_paint(ffi, case, inplace, offset)
    image = case["image"]
    assert got["rc"] == 0, ffi.lib().isegmi_last_error()
    assert (got["out"][image.size:] == PAINT_SENTINEL).all(), "bytes past H * W * 3 were written"
    if not inplace:
        assert np.array_equal(got["src"], image.reshape(-1)), "a separate output must leave the input alone"
    out = got["out"][:image.size].reshape(image.shape)
    assert np.array_equal(out, want["image"]), (profile, seed, inplace, offset, np.argwhere((out != want["image"]).any(2))[:4].tolist())
    once_again("paint", lambda: run_paint(ffi, case, inplace, offset), got)


def run_resample(ffi, case):
    views = ffi.resample_u8(case["images"], case["entries"])
    canvas = ffi.resample_u8(case["images"], case["entries"], canvas=case["canvas"], mean3=case["mean"], std3=case["std"], swap_rb=case["swap"], fill=case["fill"])
    return dict(views=views, canvas=canvas)


@settings(**SET)
@given(profile=st.sampled_from(fc.RESAMPLE_PROFILES), seed=SEED)
def test_resample_u8_both_epilogues(ffi, profile, seed):
    """the byte epilogue and the fp32 canvas epilogue of one set of views; the canvas was NaN before the launch, so an element nobody wrote shows"""
    case, want = case_of("resample", profile, seed)
    got = run_resample(ffi, case)
    assert len(got["views"]) == len(want["views"])
    for k, (g, w) in enumerate(zip(got["views"], want["views"])):
        assert g.shape == w.shape and g.dtype == np.uint8 and np.array_equal(g, w), (profile, seed, case["entries"][k], np.argwhere(g != w)[:4].tolist())
    assert same_bits(got["canvas"], want["canvas"]), (profile, seed, np.argwhere(got["canvas"].view(np.uint32) != want["canvas"].view(np.uint32))[:4].tolist())
    once_again("resample", lambda: run_resample(ffi, case), got)


# ---------------------------------------------------------------------------------------------------------------- detection tails
def same_lists(got, want):
    """(boxes, scores, labels) or (scores, indices): floats by bit pattern, integers by value"""
    return len(got) == len(want) and all((same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)) if np.asarray(w).dtype == np.float32
                                          else np.array_equal(g, w)) and np.asarray(g).shape == np.asarray(w).shape for g, w in zip(got, want))


def run_yolo_select(ffi, case):
    kw = case["kw"]
    dec, total = ffi.yolo_select(case["heads"], kw["strides"], kw["anchors"], A=kw["A"], top_n=kw["top_n"], conf_thresh=kw["thr"], multi_label=int(kw["multi_label"]),
                                 min_wh=kw["min_wh"], canvas_w=kw["canvas_w"], canvas_h=kw["canvas_h"])
    return dict(dec=dec, total=total)


@settings(**SET)
@given(profile=st.sampled_from(fc.YOLO_PROFILES), seed=SEED)
def test_yolo_select(ffi, profile, seed):
    """the fused select / decode: lists in selection order and the candidate totals before the cut; the wrapper itself holds the rows past every count to
    their fill (zero box, score -1, label 0)"""
    case, want = case_of("yolo_select", profile, seed)
    got = run_yolo_select(ffi, case)
    assert np.array_equal(got["total"], want["total"]), (profile, seed, got["total"].tolist(), want["total"].tolist())
    for l, row in enumerate(want["dec"]):
        for n, w in enumerate(row):
            assert same_lists(got["dec"][l][n], w), (profile, seed, l, n, len(got["dec"][l][n][1]), len(w[1]))
    once_again("yolo_select", lambda: run_yolo_select(ffi, case), got)


def run_retina(ffi, case):
    """select + decode, then the postprocess over the lists exactly as the select stage leaves them: nseg = nl segments of top_n slots, filled past the counts"""
    sel, dec = ffi.retina_select(case["logits"], case["A"], case["top_n"], case["thr"], case["deltas"], case["anchors"], case["image_hw"], case["min_size"])
    nl, N, T = len(dec), len(dec[0]), case["top_n"]
    B = np.zeros((N, nl, T, 4), np.float32); S = np.full((N, nl, T), -1, np.float32); L = np.zeros((N, nl, T), np.int32); cnt = np.zeros((N, nl), np.int32)
    for l in range(nl):
        for n in range(N):
            c = len(dec[l][n][1])
            B[n, l, :c], S[n, l, :c], L[n, l, :c], cnt[n, l] = dec[l][n][0], dec[l][n][1], dec[l][n][2], c
    return dict(sel=sel, dec=dec, dets=ffi.retina_postprocess(B, S, L, cnt, **case["post"]))


@settings(**SET)
@given(profile=st.sampled_from(fc.RETINA_PROFILES), seed=SEED)
def test_retina_select_decode_postprocess(ffi, profile, seed):
    case, want = case_of("retina", profile, seed)
    got = run_retina(ffi, case)
    for l in range(len(want["sel"])):
        for n in range(len(want["sel"][l])):
            assert same_lists(got["sel"][l][n], want["sel"][l][n]), (profile, seed, "select", l, n)
            assert same_lists(got["dec"][l][n], want["dec"][l][n]), (profile, seed, "decode", l, n)
    for n, w in enumerate(want["dets"]):
        assert same_lists(got["dets"][n], w), (profile, seed, "postprocess", n, len(got["dets"][n][1]), len(w[1]), case["post"])
    once_again("retina", lambda: run_retina(ffi, case), got)


YOLACT_KEYS = ("prior", "cls", "score", "box", "mask")


def run_yolact_detect(ffi, case, mode):
    p = case["params"]
    got, boxes, total, over = ffi.yolact_detect(case["conf"], case["loc"], case["mask"], case["priors"], conf_thresh=p["conf_thresh"], nms_thresh=p["nms_thr"], top_k=p["top_k"],
                                                max_det=p["max_det"], nms_mode=mode, trad_cap=p["cap"], max_size=p["max_size"], return_nms=True)
    return dict(det=[[g[k] for k in YOLACT_KEYS] for g in got], boxes=boxes, total=total, over=over)


@settings(**SET)
@given(profile=st.sampled_from(fc.YOLACT_PROFILES), seed=SEED, mode=st.sampled_from([0, 1, 2]))
def test_yolact_detect_in_every_nms_mode(ffi, profile, seed, mode):
    """fast NMS (mode 0, against the oracle), cross-class fast NMS and traditional per-class NMS under a candidate cap (modes 1 and 2, against
    tests/yolact_nms_ref.py): detections, and in modes 1 and 2 the survivor total and the cap lemma's overflow flag"""
    case = fc.build_yolact_detect(profile, seed)
    assert profile in case["reached"], (profile, seed, case["reached"])
    want = fc.ref_yolact_detect(case, (mode,))[mode]
    got = run_yolact_detect(ffi, case, mode)
    for n, (ref, rt, ro) in enumerate(want):
        for k, g in zip(YOLACT_KEYS, got["det"][n]):
            assert g.shape == ref[k].shape and (same_bits(g, ref[k]) if ref[k].dtype == np.float32 else np.array_equal(g, ref[k])), (profile, seed, mode, n, k, len(g), len(ref[k]))
        if mode:
            assert int(got["total"][n]) == rt and int(got["over"][n]) == ro, (profile, seed, mode, n, int(got["total"][n]), rt, int(got["over"][n]), ro)
    once_again("yolact_detect", lambda: run_yolact_detect(ffi, case, mode), got)


def run_bbox_aug(ffi, case):
    N = case["views"][0]["logits"].shape[0]
    pool = ffi.BBoxAugPool(N, case["cap"])
    for v in case["views"]:
        ffi.bbox_aug_candidates(pool, v["logits"], v["regr"], v["props"], v["cnt"], v["hw"], v["hflip"], np.tile(v["ratios"], (N, 1)), case["thr"], case["agnostic"])
    B, S, Lb, cnt, total = pool.numpy()
    return dict(boxes=B, scores=S, labels=Lb, cnt=cnt, total=total, dets=ffi.bbox_aug_merge(pool, case["ncls"], **case["post"]))


@settings(**SET)
@given(profile=st.sampled_from(fc.BBOX_AUG_PROFILES), seed=SEED)
def test_bbox_aug_candidate_pool_and_merge(ffi, profile, seed):
    """the views' candidates appended view-major to the capped pool, the slots past the count left poisoned, then the merge over the pool"""
    case, want = case_of("bbox_aug", profile, seed)
    got = run_bbox_aug(ffi, case)
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
    for n, ((rb, rs, rl), rtotal) in enumerate(want["pools"]):
        c = len(rs)
        assert int(got["total"][n]) == rtotal and int(got["cnt"][n]) == c == min(case["cap"], rtotal), (profile, seed, n, int(got["total"][n]), rtotal, int(got["cnt"][n]), c)
        assert np.array_equal(got["labels"][n, :c], rl) and same_bits(got["scores"][n, :c], rs) and same_bits(got["boxes"][n, :c], rb), (profile, seed, n)
        assert (u32(got["scores"][n, c:]) == 0xFFFFFFFF).all() and (got["labels"][n, c:] == -1).all() and (u32(got["boxes"][n, c:]) == 0xFFFFFFFF).all(), (profile, seed, n, "past the count")
        assert same_lists(got["dets"][n], want["dets"][n]), (profile, seed, "merge", n, len(got["dets"][n][1]), len(want["dets"][n][1]))
    once_again("bbox_aug", lambda: run_bbox_aug(ffi, case), got)
