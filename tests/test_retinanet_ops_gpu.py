"""The RetinaNet tail kernels (csrc/retinanet_ops.hip) against tests/retinanet_ref.py on the crafted inputs of tests/retinanet_cases.py, bit for bit, and the
one convolution shape the model adds.  tests/test_retinanet_cpu.py shows on the CPU that each crafted input discriminates the rule it is named for."""
import numpy as np
import pytest

import retinanet_cases as rc
import retinanet_ref as rr
from oracle import ora

pytestmark = pytest.mark.gpu
F32 = np.float32
SELECT = rc.select_cases()
POST = rc.post_cases()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _check_select(ffi, logits, a, c, top_n, thr=0.05):
    got = ffi.retina_select(logits, a, top_n, thr)
    counts = []
    for l, lg in enumerate(logits):
        for n in range(lg.shape[0]):
            s, i = rr.select_level(lg[n], top_n, thr)
            gs, gi = got[l][n]
            assert len(gs) == len(s), (l, n, len(gs), len(s))
            assert np.array_equal(gi, i), (l, n)
            assert np.array_equal(_bits(gs), _bits(s)), (l, n)
            counts.append(len(s))
    return counts


@pytest.mark.parametrize("name", sorted(SELECT))
def test_retina_select(ffi, name):
    logits, a, c, top_n = SELECT[name]
    counts = _check_select(ffi, logits, a, c, top_n)
    if name.startswith("none"):
        assert counts == [0] * len(counts)
    if name == "exactly_top_n_and_one_more":
        assert counts == [1000, 1000, 1000, 1000, 720, 1]
    if name == "every_logit_passes":
        assert counts == [1000, 1000, 1000, 1000, 720, 720]


@pytest.mark.parametrize("name", ["long_all_in_last_slice", "long_spread"])
def test_retina_select_long_row(ffi, name):
    """(40, 41, 9, 80): 1 180 800 logits = 145 slices of the kernel's 8192 (any row over 8192 logits takes the multi-slice path; the 25 200-logit rows of the
    other cases already do)."""
    logits, a, c, top_n = rc.long_cases()[name]
    assert logits[0][0].size > 100 * rc.SLICE
    assert _check_select(ffi, logits, a, c, top_n) == [1000]


def test_retina_select_is_reproducible(ffi):
    logits, a, c, top_n = SELECT["equal_run_at_cut"]
    r0 = ffi.retina_select(logits, a, top_n)
    for _ in range(3):
        r = ffi.retina_select(logits, a, top_n)
        for l in range(len(logits)):
            for n in range(2):
                assert np.array_equal(r[l][n][1], r0[l][n][1]) and np.array_equal(_bits(r[l][n][0]), _bits(r0[l][n][0]))


def test_retina_select_refuses_what_it_cannot_hold(ffi):
    logits, a, c, _ = SELECT["toy"]
    with pytest.raises(ffi.IsegmiError):
        ffi.retina_select(logits, a, 1025)


def test_retina_decode(ffi):
    logits, deltas, anchors, hw = rc.decode_case()
    sel, dec = ffi.retina_select(logits, rc.A, rc.TOP_N, 0.05, deltas, anchors, hw)
    outside = clamped = 0
    for l in range(len(logits)):
        for n in range(2):
            s, i = rr.select_level(logits[l][n])
            assert np.array_equal(sel[l][n][1], i)
            b, sc, lb = rr.decode_level(s, i, deltas[l][n], anchors[l], hw[n][1], hw[n][0])
            gb, gs, gl = dec[l][n]
            assert len(gs) == len(sc) > 0
            assert np.array_equal(_bits(gb), _bits(b)) and np.array_equal(_bits(gs), _bits(sc)) and np.array_equal(gl, lb)
            an = anchors[l][i // rc.C]; d = deltas[l][n].reshape(-1, 4)[i // rc.C]
            outside += int(((an[:, 0] < 0) | (an[:, 2] > hw[n][1] - 1)).sum())
            clamped += int((d[:, 2] / F32(5.0) >= F32(4.135166556742356)).sum())
    assert outside > 0 and clamped > 0


def test_retina_decode_min_size(ffi):
    """min_size drops boxes in place: the survivors keep their selection order."""
    logits, deltas, anchors, hw = rc.decode_case()
    _, dec = ffi.retina_select(logits, rc.A, rc.TOP_N, 0.05, deltas, anchors, hw, min_size=12.0)
    dropped = 0
    for l in range(len(logits)):
        for n in range(2):
            s, i = rr.select_level(logits[l][n])
            b, sc, lb = rr.decode_level(s, i, deltas[l][n], anchors[l], hw[n][1], hw[n][0], min_size=12.0)
            dropped += len(s) - len(sc)
            gb, gs, gl = dec[l][n]
            assert len(gs) == len(sc)
            assert np.array_equal(_bits(gb), _bits(b)) and np.array_equal(_bits(gs), _bits(sc)) and np.array_equal(gl, lb)
    assert dropped > 0


def _check_post(ffi, case, nms_flags=0, det=100, cap=128):
    B, S, Lb, cnt = rc.pack_post(case)
    got = ffi.retina_postprocess(B, S, Lb, cnt, 81, 0.4, det, cap, nms_flags)
    ref = rc.ref_post(case, nms_flags, det, cap)
    for n, (g, r) in enumerate(zip(got, ref)):
        assert len(g[1]) == len(r[1]), (n, len(g[1]), len(r[1]))
        assert np.array_equal(g[2], r[2]), n
        assert np.array_equal(_bits(g[1]), _bits(r[1])), n
        assert np.array_equal(_bits(g[0]), _bits(r[0])), n
    return [len(r[1]) for r in ref]


@pytest.mark.parametrize("name", sorted(POST))
def test_retina_postprocess(ffi, name):
    counts = _check_post(ffi, POST[name])
    if name == "identical_boxes_two_classes":
        assert counts == [2]
    if name == "cut_tie_group_fits_cap":
        assert counts == [115]
    if name == "cut_tie_group_over_cap":
        assert counts == [128]
    if name == "fewer_than_det":
        assert counts == [40, 0]
    if name == "zero_candidates":
        assert counts == [0]


@pytest.mark.parametrize("flags", [1, 2, 4, 7])
@pytest.mark.parametrize("name", ["eighty_classes_5000", "iou_exactly_thr"])
def test_retina_postprocess_forks(ffi, name, flags):
    _check_post(ffi, POST[name], nms_flags=flags)


def test_retina_postprocess_iou_at_threshold(ffi):
    assert _check_post(ffi, POST["iou_exactly_thr"], 0) == [4]      # iou == thr: kept under >
    assert _check_post(ffi, POST["iou_exactly_thr"], 1) == [2]      # suppressed under ISEGMI_NMS_GE


def test_retina_postprocess_uncut(ffi):
    """det_per_img 0: no cut; cap alone bounds the rows."""
    _check_post(ffi, POST["one_class_5000"], det=0, cap=4096)


@pytest.mark.parametrize("act", [0, 1])
def test_p6_conv_shape(ffi, act):
    """LastLevelP6P7's p6: 3x3 stride 2 pad 1 with Cin 2048 on an odd map, 5 x 7 x 2048 -> 3 x 4 x 256."""
    rng = np.random.default_rng(30)
    x = rng.standard_normal((1, 5, 7, 2048)).astype(F32)
    w = (rng.standard_normal((256, 3, 3, 2048)) * 0.02).astype(F32)
    b = rng.standard_normal(256).astype(F32)
    ref = ora.conv2d(x, w, 2, 1, None, b, None, act)
    got = ffi.conv2d(x, w, 2, 1, None, b, None, act)
    assert ref.shape == (1, 3, 4, 256)
    assert act == 0 or (ref == 0).any()
    assert np.array_equal(_bits(got), _bits(ref))
