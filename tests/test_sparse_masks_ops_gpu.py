"""The sparse-mask contract on the device, op by op and bit for bit: paste_masks_kernel and yolact_upsample_masks_kernel with clear = 0 over planes
that hold 0xA5 (then: the previous step's masks), their window outputs, and the run-length encoder reading the planes they left through the windows
they reported.  Cases, reference windows and checkers: tests/sparse_mask_cases.py (proven on the oracle by tests/test_sparse_masks_cpu.py).  Also the
ops around the Yolact assembly that only the end-to-end tests ran: the dense prototype masks, the mask-IoU net's first layer and its final re-scoring."""
import functools

import numpy as np
import pytest

import sparse_mask_cases as sc
from oracle import ora

pytestmark = pytest.mark.gpu
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _paste_ref(h, w, M, step):
    case = sc.paste_case(h, w, M, step)
    return case, sc.paste_dense(ora, case)


@functools.lru_cache(maxsize=None)
def _yolact_ref(shape, step):
    case = sc.yolact_case(*shape, step=step)
    return (case,) + sc.yolact_dense(ora, case)


def _device_encoder(ffi):
    return lambda planes, counts, image_hw, wins: ffi.rle_encode(planes, counts, image_hw, windows=wins)


def _smaller(h, w):
    """per-image sizes inside the plane for the encoder: the plane itself, a few rows and one column less, half of it"""
    return np.array([[h, w], [max(h - 3, 1), max(w - 1, 1)], [max(h // 2, 1), max(w // 2, 1)]], np.int32)


@pytest.mark.parametrize("h,w,M", [(h, w, M) for (h, w) in sc.PASTE_PLANES for M in sc.PASTE_M])
def test_paste_sparse_contract_over_two_steps(ffi, h, w, M):
    """clear = 0 over poisoned planes, then a second launch with other boxes and counts over what the first one left: the window is Masker's own
    (exactly), every set pixel lies in it, every byte in it is the oracle's, nothing else changes but the zeros of a whole-word store, slots past the
    count keep plane and window, and the encoder gets the dense masks' counts and strings out of the dirty planes; clear = 1 gives the same bytes
    inside the windows and zeros elsewhere; without a window buffer the planes are the same"""
    K = len(sc.paste_boxes(h, w, M))
    planes = np.full((sc.N_IMAGES, K, h, w), sc.POISON, np.uint8)
    wins = np.full((sc.N_IMAGES, K, 4), sc.WIN_POISON, np.int32)
    encode = _device_encoder(ffi)
    for step in (0, 1):
        case, dense = _paste_ref(h, w, M, step)
        counts, names = case["counts"], case["names"]
        before, wins_before = planes, wins
        planes, wins = ffi.paste_masks_win(case["masks"], case["boxes"], counts, h, w, 0.5, clear=False, planes=before, windows=wins_before)
        ref = sc.masker_window(case["boxes"], M, h, w)
        for n in range(sc.N_IMAGES):
            c = int(counts[n])
            assert np.array_equal(wins[n, :c], ref[n, :c]), (step, n, [(names[n][k], tuple(wins[n, k]), tuple(ref[n, k])) for k in range(c) if tuple(wins[n, k]) != tuple(ref[n, k])])
        sc.check_containment(dense, wins, counts, names)
        sc.check_coverage(planes, dense, wins, counts, names)
        sc.check_confinement(planes, before, wins, counts, names, spill=True)
        sc.check_dead_slots(planes, before, wins, wins_before, counts)
        sc.check_chain(encode, ora, planes, counts, wins, dense)
        sc.check_chain(encode, ora, planes, counts, wins, dense, _smaller(h, w))
        cleared, cwins = ffi.paste_masks_win(case["masks"], case["boxes"], counts, h, w, 0.5, clear=True, planes=before, windows=wins_before)
        sc.check_dense_equals_sparse(cleared, planes, wins, counts)
        assert np.array_equal(cwins, wins) and np.array_equal(cleared, dense)
        nowin, none = ffi.paste_masks_win(case["masks"], case["boxes"], counts, h, w, 0.5, clear=False, planes=before, want_windows=False)
        assert none is None and np.array_equal(nowin, planes)


_YOLACT_IDS = ["%dx%d-%dx%d%s" % (s[0], s[1], s[2], s[3], "-ragged" if s[4] else "") for s in sc.YOLACT_SHAPES]


@pytest.mark.parametrize("shape", sc.YOLACT_SHAPES, ids=_YOLACT_IDS)
def test_yolact_sparse_contract_over_two_steps(ffi, shape):
    """the same for the Yolact assembly, with NaN in ws_lo and per-image sizes inside the common plane: the conservative window holds every output
    pixel with a live tap and stays within 3 pixels of their bounding box; outside it not one byte changes"""
    PH, PW, h, w, ragged = shape
    planes = np.full((sc.N_IMAGES, sc.YOLACT_K, h, w), sc.POISON, np.uint8)
    wins = np.full((sc.N_IMAGES, sc.YOLACT_K, 4), sc.WIN_POISON, np.int32)
    encode = _device_encoder(ffi)
    for step in (0, 1):
        case, dense, lo = _yolact_ref(shape, step)
        counts, names, hw = case["counts"], case["names"], sc.image_sizes(case)
        args = (case["proto"], case["coeffs"], case["boxes"], counts, h, w)
        before, wins_before = planes, wins
        planes, wins, _, ib = ffi.yolact_masks_win(*args, image_hw=case["image_hw"], clear=False, planes=before, windows=wins_before)
        sc.check_yolact_window_bounds(case, wins)
        sc.check_containment(dense, wins, counts, names)
        sc.check_coverage(planes, dense, wins, counts, names)
        sc.check_confinement(planes, before, wins, counts, names, spill=False)
        sc.check_dead_slots(planes, before, wins, wins_before, counts)
        sc.check_chain(encode, ora, planes, counts, wins, dense, hw)
        if not ragged:
            sc.check_chain(encode, ora, planes, counts, wins, dense, None)
            sc.check_chain(encode, ora, planes, counts, wins, dense, _smaller(h, w))
        cleared, cwins, _, cib = ffi.yolact_masks_win(*args, image_hw=case["image_hw"], clear=True, planes=before, windows=wins_before)
        sc.check_dense_equals_sparse(cleared, planes, wins, counts)
        assert np.array_equal(cwins, wins) and np.array_equal(cleared, dense) and np.array_equal(cib, ib)
        nowin, none, _, _ = ffi.yolact_masks_win(*args, image_hw=case["image_hw"], clear=False, planes=before, want_windows=False)
        assert none is None and np.array_equal(nowin, planes)
        if not ragged:   # image_hw = NULL and image_hw = the plane's size are the same fork-free result
            same, swins, _, _ = ffi.yolact_masks_win(*args, image_hw=np.tile(np.array([[h, w]], np.int32), (sc.N_IMAGES, 1)), clear=False, planes=before,
                                                     windows=wins_before)
            assert np.array_equal(same, planes) and np.array_equal(swins, wins)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("shape", sc.YOLACT_SHAPES, ids=_YOLACT_IDS)
def test_yolact_proto_stage_dense_and_sparse(ffi, shape):
    """dense_lo = 1 (what YOLACT++'s mask-IoU net reads): every element of a live slot is the oracle's cropped prototype mask, no NaN of the poisoned
    workspace is left; dense_lo = 0: the crop's elements are, the rest keeps its NaN; slots past the count keep theirs; the planes do not differ"""
    PH, PW, h, w, ragged = shape
    case, dense, lo = _yolact_ref(shape, 0)
    args = (case["proto"], case["coeffs"], case["boxes"], case["counts"], h, w)
    p1, w1, lo1, _ = ffi.yolact_masks_win(*args, image_hw=case["image_hw"], clear=False, dense_lo=True)
    p0, w0, lo0, _ = ffi.yolact_masks_win(*args, image_hw=case["image_hw"], clear=False, dense_lo=False)
    assert np.array_equal(p1, p0) and np.array_equal(w1, w0)
    yy, xx = np.mgrid[0:PH, 0:PW].astype(F32)
    n_out = 0
    for n in range(sc.N_IMAGES):
        c = int(case["counts"][n])
        assert np.isnan(lo1[n, c:]).all() and np.isnan(lo0[n, c:]).all(), n
        for k in range(c):
            assert not np.isnan(lo1[n, k]).any() and np.array_equal(_bits(lo1[n, k]), _bits(lo[n, k])), (n, k, case["names"][n][k])
            x1, x2, y1, y2 = sc.yolact_crop(case["boxes"][n, k], PH, PW)
            inside = (xx >= x1) & (xx < x2) & (yy >= y1) & (yy < y2)
            assert np.array_equal(_bits(lo0[n, k][inside]), _bits(lo[n, k][inside])) and np.isnan(lo0[n, k][~inside]).all(), (n, k, case["names"][n][k])
            assert not lo[n, k][~inside].any()
            n_out += int((~inside).sum())
    assert n_out > 0


@pytest.mark.parametrize("PH,PW", [(3, 3), (4, 5), (9, 8), (23, 31)])
def test_maskiou_conv1_matches_its_fmaf_chain(ffi, PH, PW):
    """channels 0..7 bit-identical to the nine-term fmaf chain + bias + ReLU restated in numpy fp32, and within gamma(11) (sum |x w| + |b|) of the fp64
    value (nine fused multiply-adds, the bias and the + 0: one rounding each, u = 2^-24); channels 8..31 exactly +0 over a NaN-filled output"""
    rng = np.random.default_rng(PH * 100 + PW)
    NK = 5
    lo = (rng.uniform(0, 1, (NK, PH, PW)) * (rng.uniform(0, 1, (NK, PH, PW)) < 0.7)).astype(F32)   # sigmoid values and the crop's zeros
    lo[0] = 1.0
    w = rng.standard_normal((8, 9)).astype(F32); b = (rng.standard_normal(8) * 0.5).astype(F32)
    w[7] = -np.abs(w[7]); b[7] = -0.25                                                         # a channel the ReLU zeroes everywhere
    out = ffi.maskiou_conv1(lo, w, b)
    ref, exact, mag = sc.maskiou_conv1_ref(lo, w, b)
    Ho, Wo = (PH - 3) // 2 + 1, (PW - 3) // 2 + 1
    assert out.shape == (NK, Ho, Wo, 32) and ref.shape == (NK, Ho, Wo, 8)
    assert not _bits(out[..., 8:]).any()
    assert np.array_equal(_bits(out[..., :8]), _bits(ref))
    u = 2.0 ** -24
    err = np.abs(out[..., :8].astype(np.float64) - np.maximum(exact, 0.0))
    assert (err <= 11 * u / (1 - 11 * u) * mag).all(), float((err / mag).max())
    assert (ref[..., :7] > 0).any() and not ref[..., 7].any()


@pytest.mark.parametrize("N,K,HW,C", [(3, 5, 1, 1), (3, 5, 1, 80), (2, 7, 12, 80), (3, 130, 4, 9)])
def test_maskiou_rescore_is_score_times_the_exact_maximum(ffi, N, K, HW, C):
    rng = np.random.default_rng(N * 1000 + K * 10 + HW)
    feat = rng.standard_normal((N, K, HW, C)).astype(F32)
    cls = rng.integers(0, C, (N, K)).astype(np.int32)
    cls[:, 0] = 0; cls[:, 1] = C - 1
    score = rng.uniform(0.05, 1.0, (N, K)).astype(F32)
    count = np.array([K, 0, K - 2][:N], np.int32)
    out = ffi.maskiou_rescore(feat, cls, score, count)
    best = np.take_along_axis(feat, cls[:, :, None, None].astype(np.int64), 3)[..., 0].max(2)        # max is exact: it returns one of its inputs
    want = np.where(np.arange(K)[None, :] < count[:, None], score * best, F32(0.0)).astype(F32)
    assert np.array_equal(_bits(out), _bits(want)), np.argwhere(out != want)[:4].tolist()
    if HW > 1:   # the maximum is not the first position's value everywhere: the loop over HW matters
        assert (best != np.take_along_axis(feat, cls[:, :, None, None].astype(np.int64), 3)[..., 0][:, :, 0]).any()
