"""The RetinaNet tail kernels (csrc/retinanet_ops.hip) against tests/retinanet_ref.py on the crafted inputs of tests/retinanet_cases.py, bit for bit, and the
one convolution shape the model adds.  tests/test_retinanet_cpu.py shows on the CPU that each crafted input discriminates the rule it is named for, or
reaches the limit it is named for: top_n 1..1024, the slice borders, 8192 slots, 255 classes, the pre-filter over the threshold range."""
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


# ---- top_n, slice borders, geometry, thresholds, decode edges (each case is shown to reach its edge in tests/test_retinanet_cpu.py)
@pytest.mark.parametrize("name", ["topn_%d" % k for k in rc.TOP_NS] + ["topn_1024_exact"])
def test_retina_select_top_n(ffi, name):
    logits, a, c, top_n = rc.topn_cases()[name]
    assert _check_select(ffi, logits, a, c, top_n) == [top_n] * 4


@pytest.mark.parametrize("kind", ["distinct", "tie"])
@pytest.mark.parametrize("n", rc.BORDER_ROWS)
def test_retina_select_slice_borders(ffi, n, kind):
    logits, a, c, top_n = rc.border_cases()["border_%s_%d" % (kind, n)]
    counts = _check_select(ffi, logits, a, c, top_n)
    assert counts == [min(64, rc.candidates(logits[0][0])), 1]


def test_retina_select_five_levels_three_images(ffi):
    logits, a, c, top_n = rc.geometry_case()
    counts = _check_select(ffi, logits, a, c, top_n)
    assert counts == [min(top_n, lg[0].size if rc.geometry_kind(l, n) < 0 else rc.geometry_kind(l, n), lg[0].size) for l, lg in enumerate(logits) for n in range(3)]


@pytest.mark.parametrize("thr", rc.THRESHOLDS)
def test_retina_select_thresholds(ffi, thr):
    """The pre-filter may only drop what the sigmoid test drops: the row holds the floats around the crossing of thr, a grid around logit(thr) - 0.25 and the
    special logits.  With the pre-filter as first built (`x > logit(thr) - 0.25` for 0 < thr < 1, `x > -inf` otherwise) this test returned 7 of the 8 numbers
    at thr -1 and 0 (the -inf logit was lost to `-inf > -inf`) and 261 of 520 at thr 1e-45 and 1e-40, which lie under the sigmoid's floor of 4.2e-39: every
    logit at or under the pre-filter was dropped although its sigmoid exceeds thr.  The other eleven thresholds passed."""
    logits, a, c, top_n = rc.threshold_case(thr)
    counts = _check_select(ffi, logits, a, c, top_n, thr)
    assert counts == [rc.candidates(logits[0], thr)]


def _check_decode(ffi, case, min_size=0.0):
    logits, deltas, anchors, hw = case
    sel, dec = ffi.retina_select(logits, rc.A, rc.TOP_N, 0.05, deltas, anchors, hw, min_size=float(min_size))
    kept = []
    for l in range(len(logits)):
        for n in range(2):
            s, i = rr.select_level(logits[l][n])
            assert np.array_equal(sel[l][n][1], i)
            b, sc, lb = rr.decode_level(s, i, deltas[l][n], anchors[l], hw[n][1], hw[n][0], min_size=min_size)
            gb, gs, gl = dec[l][n]
            assert len(gs) == len(sc), (l, n, len(gs), len(sc))
            assert np.array_equal(_bits(gb), _bits(b)) and np.array_equal(_bits(gs), _bits(sc)) and np.array_equal(gl, lb)
            kept.append((len(s), len(sc)))
    return kept


def test_retina_decode_one_pixel_image(ffi):
    assert all(k == m > 0 for k, m in _check_decode(ffi, rc.decode_edge_case("tiny_image")))


def test_retina_decode_min_size_edge(ffi):
    """min_size equal to a box's side + 1 keeps it (>=), the next float drops it; a min_size over every box leaves counts of 0 and filled rows."""
    case = rc.decode_edge_case("zero_deltas")
    m, m_up = rc.min_size_edge()
    at, up = _check_decode(ffi, case, m), _check_decode(ffi, case, m_up)
    assert up[0][1] < at[0][1] < at[0][0]
    assert all(m == 0 and k > 0 for k, m in _check_decode(ffi, case, 1e9))


def test_retina_decode_special_deltas(ffi):
    """NaN in dx / dy makes a NaN box, dropped by the size test; +-inf clips to the border; a NaN dw takes the clamp's value."""
    assert all(k - m >= 2 for k, m in _check_decode(ffi, rc.decode_edge_case("special_deltas")))


def _check_post(ffi, case, nms_flags=0, det=100, cap=128, ref=None):
    B, S, Lb, cnt = rc.pack_post(case)
    got = ffi.retina_postprocess(B, S, Lb, cnt, case.get("ncls", 81), 0.4, det, cap, nms_flags)
    ref = rc.ref_post(case, nms_flags, det, cap) if ref is None else ref
    assert len(got) == len(ref)
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


# ---- capacity, class range and the cut's edges (tests/test_retinanet_cpu.py: test_full_cases_reach_the_capacity, test_edge_post_cases_discriminate)
@pytest.mark.parametrize("det, cap", [(100, 128), (0, 8192)])
@pytest.mark.parametrize("name", ["full_one_class", "full_100_then_8092", "full_255_classes", "batch_8192_0_1"])
def test_retina_postprocess_full(ffi, name, det, cap):
    """All 8192 slots (the 13-bit slot field full, 128 matrix words per row): one class over 128 words; a class that starts inside a word and spans 127;
    labels 254 / 255 of ncls 256 with a class of 65 words from word 63; 8192, 0 and 1 candidates in one launch."""
    counts = _check_post(ffi, rc.full_cases()[name], det=det, cap=cap, ref=rc.full_ref(name, det, cap))
    assert counts[0] >= 100 if det else counts[0] > 1000
    if name == "batch_8192_0_1":
        assert counts[1:] == [0, 1]


@pytest.mark.parametrize("name", ["ncls_2", "labels_out_of_range_ncls_2", "labels_out_of_range_ncls_81"])
def test_retina_postprocess_class_range(ffi, name):
    counts = _check_post(ffi, rc.edge_post_cases()[name])
    assert counts == [6] or name == "ncls_2"


@pytest.mark.parametrize("name, dets, counts", [("cut_k40", (1, 39, 40, 41, 0), (1, 40, 40, 40, 40)), ("cut_k40_zeros", (1, 32, 39, 40, 41, 0), (1, 34, 40, 40, 40, 40))])
def test_retina_postprocess_cut_edges(ffi, name, dets, counts):
    """det_per_img 1, one under the number kept (the tie at the cut keeps both), the number kept, one over; a cut inside a group of +0.0 and -0.0."""
    for det, want in zip(dets, counts):
        assert _check_post(ffi, rc.edge_post_cases()[name], det=det, cap=64) == [want], det
    for flags in (4, 7):
        _check_post(ffi, rc.edge_post_cases()[name], nms_flags=flags, det=39, cap=64)


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
