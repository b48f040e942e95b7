"""The Keypoint R-CNN engine in every launch form (tests/test_keypointrcnn_gpu.py runs the default form, graph replay and short batches): the
stream / grouping / aliasing / RPN-selection parameters, the head's two RoIAlign launches (`roi_table` bit 1), hipGraph with the plain RoIAlign, a canvas
change on one engine, ROIAlign(aligned=True), and an image whose detections fill every slot next to an image with none.  The 128 x 160 canvas, the seeded
weights and the threshold of tests/test_keypointrcnn_gpu.py; every run is two forwards and the second must equal the first; bit for bit throughout."""
import ctypes as C

import numpy as np
import pytest

import fasterrcnn_cases as fc
import keypoint_ref as kr
from conv_ref import same_bits
from oracle import ora
from test_keypointrcnn_gpu import FX, _batch, _cfg, _sd

pytestmark = pytest.mark.gpu

KEYS = fc.DET_KEYS + ("det.kpt", "det.kscore")
CAP = 100

VARIANTS = [dict(multi_stream=0), dict(conv_groups=0), dict(multi_stream=0, conv_groups=0), dict(alias_buffers=0), dict(rpn_select_groups=0),
            dict(rpn_select_groups=2), dict(rpn_select_on_tail=0), dict(roi_table=0), dict(roi_table=1), dict(roi_table=2), dict(roi_table=3),
            dict(graph=1, roi_table=0)]


def _model(H, W, cfg, max_batch, params=()):
    from isegmi.maskrcnn import MaskRCNN
    m = MaskRCNN(_sd(), H, W, cfg=cfg, max_batch=max_batch)
    for k, v in dict(params).items():
        m.set_param(k, float(v))
    return m


def _fetch(m, n):
    out = {k: m.fetch(k, n).copy() for k in KEYS}
    cap = out["det.box"].shape[1]
    heat = m.fetch("kp.heat", n * cap)   # rows given: a graph replay runs no host code, so the buffer's recorded shape is the last eager forward's
    assert heat.shape == (n * cap, 56, 56, 17)
    out["kp.heat"] = [heat[i * cap:i * cap + int(c)].copy() for i, c in enumerate(out["det.count"])]   # live slots: the others hold what the convolutions made of stale rows
    return out


def _forward_twice(m, x, hw):
    n = m.upload(x, hw)
    m.forward_device(n); m.sync()
    first = _fetch(m, n)
    m.forward_device(n); m.sync()
    _same(_fetch(m, n), first, "second forward")
    return first


def _same(a, b, what):
    for k in KEYS:
        assert same_bits(a[k], b[k]), (what, k)
    assert len(a["kp.heat"]) == len(b["kp.heat"])
    for i, (u, v) in enumerate(zip(a["kp.heat"], b["kp.heat"])):
        assert same_bits(u, v), (what, "kp.heat", i)


def _graph_stats(ffi, m):
    cap, rep, fail = C.c_int64(), C.c_int64(), C.c_int64()
    ffi.check(ffi.lib().isegmi_engine_graph_stats(m._h, C.byref(cap), C.byref(rep), C.byref(fail)))
    return cap.value, rep.value, fail.value


@pytest.fixture(scope="module")
def base(ffi):
    """The default engine's results at N = 2 and N = 1"""
    x, hw = _batch()
    m = _model(128, 160, _cfg(), 2)
    out = {n: _forward_twice(m, x[:n], hw[:n]) for n in (2, 1)}
    m.close()
    assert (out[2]["det.count"] > 5).all() and all(h.any() for h in out[2]["kp.heat"])
    return out


@pytest.mark.parametrize("params", VARIANTS, ids=[",".join("%s=%d" % kv for kv in v.items()) for v in VARIANTS])
def test_keypoint_launch_forms_are_bit_identical(ffi, base, params):
    x, hw = _batch()
    m = _model(128, 160, _cfg(), 2, params)
    try:
        for n in (2, 1):
            _same(_forward_twice(m, x[:n], hw[:n]), base[n], (params, n))
        if params.get("graph"):
            _same(_forward_twice(m, x[:2], hw[:2]), base[2], (params, "replay"))
            cap, rep, fail = _graph_stats(ffi, m)
            assert cap >= 2 and rep >= 2 and fail == 0, (cap, rep, fail)
    finally:
        m.close()


def test_keypoint_canvas_change_eager_and_graph(ffi, base):
    """An engine built for 256 x 352 serves that canvas (two images), then 128 x 160 (one image: every buffer of the head was sized by the larger canvas and
    the larger batch), then the large canvas again; then the same under hipGraph, whose graphs are per canvas.  Against engines built for each canvas."""
    from isegmi.maskrcnn import prepare_images
    xb, hwb = prepare_images(fc.small_images())
    xs, hws = _batch()
    xs, hws = xs[:1], hws[:1]
    assert xb.shape == (2, 256, 352, 3) and xs.shape == (1, 128, 160, 3)
    ref = _model(256, 352, _cfg(), 2)
    big = _forward_twice(ref, xb, hwb)
    ref.close()
    assert (big["det.count"] > 5).all()
    m = _model(256, 352, _cfg(), 2)
    try:
        _same(_forward_twice(m, xb, hwb), big, "large canvas")
        _same(_forward_twice(m, xs, hws), base[1], "small canvas after the large one")
        _same(_forward_twice(m, xb, hwb), big, "large canvas after the small one")
        m.set_param("graph", 1.0)
        replays = []
        for name, x, hw, want in (("big", xb, hwb, big), ("tiny", xs, hws, base[1]), ("big", xb, hwb, big)):
            _same(_forward_twice(m, x, hw), want, "graph = 1, %s, step %d" % (name, len(replays)))
            cap, rep, fail = _graph_stats(ffi, m)
            assert fail == 0, (cap, rep, fail)
            replays.append(rep)
        assert replays[0] >= 1 and replays[1] > replays[0] and replays[2] > replays[1], replays   # each canvas was replayed from its graph
    finally:
        m.close()


def test_roi_aligned_head(ffi, base):
    """ROI_ALIGNED = 1: kp.roi_feat is ROIAlign(aligned=True) of the engine's own detections (and not the legacy form of them), and the decode follows."""
    x, hw = _batch()
    m = _model(128, 160, _cfg(ROI_ALIGNED=1), 2)
    try:
        got = _forward_twice(m, x[:2], hw[:2])
        cnt = got["det.count"]
        assert (cnt > 5).all()
        P = [m.fetch(k, 2) for k in ("P2", "P3", "P4", "P5")]
        roi = m.fetch("kp.roi_feat")
        differs = 0
        for n in range(2):
            D = int(cnt[n])
            assert same_bits(roi[n * CAP:n * CAP + D], kr.roi_features(P, got["det.box"][n, :D], n, aligned=1)), n
            differs += int(not same_bits(roi[n * CAP:n * CAP + D], kr.roi_features(P, got["det.box"][n, :D], n, aligned=0)))
        assert differs == 2
        heat = m.fetch("kp.heat")
        want_kpt, want_ks = kr.decode(heat, got["det.box"], cnt)
        assert same_bits(got["det.kpt"], want_kpt) and same_bits(got["det.kscore"], want_ks)
        assert not same_bits(got["kp.heat"][0][:3], base[2]["kp.heat"][0][:3])
    finally:
        m.close()


def test_full_image_next_to_an_empty_one(ffi, base):
    """count == cap and count == 0 in one batch.  The default run's scores choose the images and the threshold: image b is the one whose best score is lowest,
    image a another one with scores above it, the threshold lies between b's best and a's next score above it (the per-class NMS goes down the scores, so
    what it keeps above a threshold does not depend on what lies below), and DETECTIONS_PER_IMG is lowered to at most four of a's detections above it.
    The last slot of the full image is then checked stage by stage as test_keypoint_head_stage_by_stage checks it."""
    from isegmi.maskrcnn import pack_keypoint_deconv
    from isegmi.weights import to_krsc
    x, hw = _batch()
    sc = [np.sort(base[2]["det.score"][n, :int(base[2]["det.count"][n])])[::-1] for n in range(2)]
    b = int(np.argmin([s[0] for s in sc]))
    a = 1 - b
    above = sc[a][sc[a] > sc[b][0]]
    assert len(above) >= 1, (sc[a][:3], sc[b][:3])
    thresh = np.float32((np.float64(above[-1]) + np.float64(sc[b][0])) / 2)
    assert sc[b][0] < thresh < above[-1]
    cap = min(len(above), 4)
    sd = _sd()
    m = _model(128, 160, _cfg(ROI_SCORE_THRESH=float(thresh), DETECTIONS_PER_IMG=cap), 2)
    try:
        order = [a, b]
        got = _forward_twice(m, x[order], np.asarray(hw)[order])
        print("threshold %.6f, detections per image %d, counts %s" % (thresh, cap, got["det.count"].tolist()))
        assert got["det.count"].tolist() == [cap, 0] and got["det.kpt"].shape == (2, cap, 17, 3)
        assert not got["det.kpt"][1].any() and not got["det.kscore"][1].any() and not got["det.box"][1].any()
        ia = [int(i) for i in np.argsort(-base[2]["det.score"][a, :int(base[2]["det.count"][a])], kind="stable")[:cap]]
        ig = np.argsort(-got["det.score"][0], kind="stable")
        assert same_bits(got["det.box"][0][ig], base[2]["det.box"][a][ia]) and same_bits(got["det.kpt"][0][ig], base[2]["det.kpt"][a][ia])   # the default run's best
        last = cap - 1
        P = [m.fetch(k, 2) for k in ("P2", "P3", "P4", "P5")]
        roi = m.fetch("kp.roi_feat")
        assert same_bits(roi[:cap], kr.roi_features(P, got["det.box"][0], 0))
        BANDS = ((0, 5, 0, 4), (4, 10, 5, 9), (9, 14, 10, 14))
        prev = roi
        for i in range(1, 9):
            cur = m.fetch("kp.fcn%d" % i)
            assert cur.shape == (2 * cap, 14, 14, 512)
            ia_, ib, oa, ob = BANDS[i % 3]
            w, bias = to_krsc(sd["%s%d.weight" % (FX, i)]), sd["%s%d.bias" % (FX, i)]
            band = ora.conv2d(prev[last:last + 1, ia_:ib], w, 1, 1, None, bias, None, 1)[0]
            assert same_bits(cur[last, oa:ob], band[oa - ia_:ob - ia_]), (i, oa)
            prev = cur
        low = m.fetch("kp.lowres68")
        w3, b4 = pack_keypoint_deconv(sd["roi_heads.keypoint.predictor.kps_score_lowres.weight"], sd["roi_heads.keypoint.predictor.kps_score_lowres.bias"])
        assert same_bits(low[last:last + 1], ora.conv2d(prev[last:last + 1], w3, 1, 1, None, b4, None, 0))
        heat = m.fetch("kp.heat")
        assert heat.shape == (2 * cap, 56, 56, 17) and same_bits(heat[:cap], kr.heatmap(low[:cap], 17))
        want_kpt, want_ks = kr.decode(heat, got["det.box"], got["det.count"])
        assert same_bits(got["det.kpt"], want_kpt) and same_bits(got["det.kscore"], want_ks)
    finally:
        m.close()
