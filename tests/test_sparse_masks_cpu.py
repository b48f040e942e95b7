"""The sparse-mask cases of tests/sparse_mask_cases.py reach what they are named for, proven on the oracle; the contract checkers pass on numpy models
of the two writers and each of them fails on a model that breaks its point.  No GPU: tests/test_sparse_masks_ops_gpu.py runs the same checkers on the
device's planes and windows."""
from fractions import Fraction

import numpy as np
import pytest

import sparse_mask_cases as sc
from oracle import ora

PASTE_PARAMS = [(h, w, M) for (h, w) in sc.PASTE_PLANES for M in sc.PASTE_M]


def _poisoned(shape):
    return np.full(shape, sc.POISON, np.uint8)


def _slots(case, names):
    """(n, k, name) of the live slots that hold one of `names`"""
    return [(n, k, nm) for n in range(sc.N_IMAGES) for k, nm in enumerate(case["names"][n]) if nm in names and k < case["counts"][n]]


# ------------------------------------------------------------------------------------------------------------------ paste: the cases
@pytest.mark.parametrize("h,w,M", PASTE_PARAMS)
def test_paste_boxes_give_the_windows_they_were_built_for(h, w, M):
    case = sc.paste_case(h, w, M)
    ref = sc.masker_window(case["boxes"], M, h, w)
    seen = 0
    for n in range(sc.N_IMAGES):
        for k, u in enumerate(case["unclamped"][n]):
            if u is not None:
                want = (max(u[0], 0), max(u[1], 0), min(u[2], w), min(u[3], h))
                assert tuple(ref[n, k]) == want, (case["names"][n][k], tuple(ref[n, k]), want)
                seen += 1
    assert seen >= 3 * 6 and np.isfinite(case["boxes"]).all()
    assert sorted(set(case["counts"]) | set(sc.paste_case(h, w, M, 1)["counts"])) == sorted({0, 1, len(case["names"][0]) - 1, len(case["names"][0])})


@pytest.mark.parametrize("h,w,M", PASTE_PARAMS)
def test_paste_border_cases_set_a_pixel_on_every_edge_of_the_window(h, w, M):
    """a window reported one pixel short on any side would leave a set pixel outside it"""
    case = sc.paste_case(h, w, M)
    dense = sc.paste_dense(ora, case)
    ref = sc.masker_window(case["boxes"], M, h, w)
    slots = _slots(case, sc.PASTE_BORDER)
    assert len(slots) >= (1 if w < 3 else 8)
    for n, k, nm in slots:
        x0, y0, x1, y1 = (int(v) for v in ref[n, k])
        p = dense[n, k]
        assert x1 > x0 and y1 > y0, nm
        assert p[y0, x0:x1].any() and p[y1 - 1, x0:x1].any() and p[y0:y1, x0].any() and p[y0:y1, x1 - 1].any(), (nm, (x0, y0, x1, y1))
        for cut in ((x0 + 1, y0, x1, y1), (x0, y0 + 1, x1, y1), (x0, y0, x1 - 1, y1), (x0, y0, x1, y1 - 1)):
            w1 = ref.copy(); w1[n, k] = cut
            with pytest.raises(AssertionError, match="set pixel outside"):
                sc.check_containment(dense, w1, case["counts"], case["names"])
    sc.check_containment(dense, ref, case["counts"], case["names"])


@pytest.mark.parametrize("h,w,M", PASTE_PARAMS)
def test_paste_windows_cover_the_named_geometries(h, w, M):
    case = sc.paste_case(h, w, M)
    dense = sc.paste_dense(ora, case)
    ref = sc.masker_window(case["boxes"], M, h, w)
    for n, k, nm in _slots(case, sc.PASTE_EMPTY):
        x0, y0, x1, y1 = ref[n, k]
        assert (x1 <= x0 or y1 <= y0) and not dense[n, k].any(), nm
        if nm in sc.PASTE_BOTH_NEGATIVE:
            assert x1 < x0 and y1 < y0 and (x1 - x0 + 3) // 4 + 1 < 0, nm      # the kernel's words-per-row is negative too: items > 0
    if w >= 16:
        assert len(_slots(case, sc.PASTE_BOTH_NEGATIVE)) >= 2
        full = [tuple(ref[n, k]) for n, k, nm in _slots(case, ("full", "over_all"))]
        assert full and all(f == (0, 0, w, h) for f in full)
        one = _slots(case, ("one_pixel",))[0]
        assert tuple(ref[one[0], one[1]]) == (5, 6, 6, 7)
        rev = _slots(case, ("reversed",))[0]
        assert ref[rev[0], rev[1], 2] <= ref[rev[0], rev[1], 0]
    if h >= 130:   # windows that start beyond the encoder's chunk 0 and end exactly on a chunk boundary
        got = {nm: tuple(ref[n, k]) for n, k, nm in _slots(case, ("chunk1_to_128", "ends_on_64", "one_row_64", "bottom_from_chunk1", "ends_on_192", "chunk1_only"))}
        assert got["chunk1_to_128"][1::2] == (70, 128) and got["ends_on_64"][3] == 64 and got["one_row_64"][1::2] == (64, 65)
        assert got["bottom_from_chunk1"][1::2] == (100, h)
        if h >= 200:
            assert got["ends_on_192"][1::2] == (130, 192) and got["chunk1_only"][1::2] == (64, 128)


@pytest.mark.parametrize("h,w,M", [p for p in PASTE_PARAMS if p[1] >= 16])
def test_paste_bottom_row_cases_close_a_run_in_row_0_of_column_x1(h, w, M):
    case = sc.paste_case(h, w, M)
    dense = sc.paste_dense(ora, case)
    ref = sc.masker_window(case["boxes"], M, h, w)
    inner, edge = _slots(case, sc.PASTE_BOTTOM_INNER), _slots(case, sc.PASTE_BOTTOM_EDGE)
    assert inner and edge
    for n, k, nm in inner:
        x0, y0, x1, y1 = (int(v) for v in ref[n, k])
        assert y1 == h and x1 < w and dense[n, k, h - 1, x1 - 1] == 1 and dense[n, k, 0, x1] == 0, nm
        ends = np.cumsum(ora.rle_encode(dense[n, k]).astype(np.int64))
        assert x1 * h in ends[1::2], nm              # a run of ones ends exactly at the first pixel of column x1
    for n, k, nm in edge:
        x0, y0, x1, y1 = (int(v) for v in ref[n, k])
        assert y1 == h and x1 == w and dense[n, k, h - 1, w - 1] == 1, nm
        assert len(ora.rle_encode(dense[n, k])) % 2 == 0, nm     # the last run is a run of ones: it closes at h * w


@pytest.mark.parametrize("h,w,M", PASTE_PARAMS)
def test_paste_poison_discriminates(h, w, M):
    """a plane that keeps 0xA5 outside the window encodes to other counts when it is read whole: an encoder that looked outside would be caught"""
    case = sc.paste_case(h, w, M)
    dense = sc.paste_dense(ora, case)
    ref = sc.masker_window(case["boxes"], M, h, w)
    planes, wins = sc.model_paste(case, dense, _poisoned(dense.shape), np.full(ref.shape, sc.WIN_POISON, np.int32))
    n_disc = 0
    for n in range(sc.N_IMAGES):
        for k in range(int(case["counts"][n])):
            if not (planes[n, k] == sc.POISON).any():    # the window (with the paste's whole-word spill on the narrow planes) is the whole plane
                continue
            assert not np.array_equal(ora.rle_encode(planes[n, k]), ora.rle_encode(dense[n, k])), case["names"][n][k]
            n_disc += 1
    assert n_disc >= (6 if w >= 16 else 1)


# ------------------------------------------------------------------------------------------------------------------ paste: the model and its mutants
def _paste_two_steps(h, w, M, mutate=None, which=("containment", "coverage", "confinement", "dead", "chain")):
    planes = _poisoned((sc.N_IMAGES, len(sc.paste_boxes(h, w, M)), h, w))
    wins = np.full(planes.shape[:2] + (4,), sc.WIN_POISON, np.int32)
    encode = sc.windowed_encoder(ora)
    for step in (0, 1):
        case = sc.paste_case(h, w, M, step)
        dense = sc.paste_dense(ora, case)
        before, wins_before = planes, wins
        planes, wins = sc.model_paste(case, dense, before, wins_before, mutate)
        if "containment" in which: sc.check_containment(dense, wins, case["counts"], case["names"])
        if "coverage" in which: sc.check_coverage(planes, dense, wins, case["counts"], case["names"])
        if "confinement" in which: sc.check_confinement(planes, before, wins, case["counts"], case["names"], spill=True)
        if "dead" in which: sc.check_dead_slots(planes, before, wins, wins_before, case["counts"])
        if "chain" in which:
            sc.check_chain(encode, ora, planes, case["counts"], wins, dense)
            hw = np.array([[h, w], [max(h - 3, 1), max(w - 1, 1)], [max(h // 2, 1), max(w // 2, 1)]], np.int32)
            sc.check_chain(encode, ora, planes, case["counts"], wins, dense, hw)
        cleared, cw = sc.model_paste(case, dense, np.zeros_like(planes), wins_before, mutate)
        if mutate is None:
            sc.check_dense_equals_sparse(cleared, planes, wins, case["counts"])
            for n in range(sc.N_IMAGES):
                c = int(case["counts"][n])
                assert np.array_equal(wins[n, :c], sc.masker_window(case["boxes"][n, :c], M, h, w))


@pytest.mark.parametrize("h,w,M", PASTE_PARAMS)
def test_paste_model_keeps_the_contract_over_two_steps(h, w, M):
    _paste_two_steps(h, w, M)


@pytest.mark.parametrize("mutate,checker,msg", [
    ("window_short_column", "containment", "set pixel outside the reported window"),
    ("window_short_column", "chain", "through the window"),
    ("skip_last_word", "coverage", "byte inside the window differs"),
    ("skip_last_word", "chain", "through the window"),
    ("clear_rows", "confinement", "byte outside the window was written"),
    ("write_dead", "dead", "slot past the count was written"),
])
def test_paste_mutants_fail_their_checker(mutate, checker, msg):
    with pytest.raises(AssertionError, match=msg):
        _paste_two_steps(13, 18, 28, mutate, (checker,))


def test_spill_mask_is_three_bytes_in_flat_order():
    m = sc.paste_spill_mask((2, 1, 4, 3), 4, 6)       # rows 1 and 2, columns 2 and 3 of a 4 x 6 plane: flat 8, 9 and 14, 15
    assert sorted(np.nonzero(m.reshape(-1))[0]) == [5, 6, 7, 10, 11, 12, 13, 16, 17, 18]
    assert not sc.paste_spill_mask((3, 3, 1, 1), 4, 6).any()


# ------------------------------------------------------------------------------------------------------------------ Yolact
@pytest.mark.parametrize("shape", sc.YOLACT_SHAPES, ids=lambda s: "%dx%d-%dx%d%s" % (s[0], s[1], s[2], s[3], "-ragged" if s[4] else ""))
def test_yolact_cases_and_model_keep_the_contract_over_two_steps(shape):
    planes = _poisoned((sc.N_IMAGES, sc.YOLACT_K, shape[2], shape[3]))
    wins = np.full((sc.N_IMAGES, sc.YOLACT_K, 4), sc.WIN_POISON, np.int32)
    encode = sc.windowed_encoder(ora)
    for step in (0, 1):
        case = sc.yolact_case(*shape, step=step)
        assert np.isfinite(case["boxes"]).all()
        dense, lo = sc.yolact_dense(ora, case)
        hw = sc.image_sizes(case)
        before, wins_before = planes, wins
        planes, wins = sc.model_yolact(case, dense, before, wins_before)
        sc.check_yolact_window_bounds(case, wins)
        sc.check_containment(dense, wins, case["counts"], case["names"])
        sc.check_coverage(planes, dense, wins, case["counts"], case["names"])
        sc.check_confinement(planes, before, wins, case["counts"], case["names"], spill=False)
        sc.check_dead_slots(planes, before, wins, wins_before, case["counts"])
        sc.check_chain(encode, ora, planes, case["counts"], wins, dense, hw)
        # the named geometries: nothing set for the boxes wholly outside; the solid boxes fill their crop up to the image's last row / column
        for n, k, nm in _slots(case, sc.YOLACT_EMPTY):
            assert not dense[n, k].any() and not lo[n, k].any(), nm
        for n, k, nm in _slots(case, sc.YOLACT_BOTTOM + sc.YOLACT_BOTTOM_EDGE):
            hn, wn = int(hw[n, 0]), int(hw[n, 1])
            assert dense[n, k, hn - 1, :wn].any(), nm
            if nm in sc.YOLACT_BOTTOM_EDGE:
                assert dense[n, k, hn - 1, wn - 1] == 1, nm
        # every set pixel has a live tap on both axes: the tap set is what the window has to hold
        for n in range(sc.N_IMAGES):
            for k in range(int(case["counts"][n])):
                bx, by = sc.yolact_tap_bounds(case["boxes"][n, k], case["PH"], case["PW"], int(hw[n, 0]), int(hw[n, 1]))
                ys, xs = np.nonzero(dense[n, k])
                if ys.size:
                    assert bx and by and bx[0] <= xs.min() and xs.max() < bx[1] and by[0] <= ys.min() and ys.max() < by[1], case["names"][n][k]


@pytest.mark.parametrize("mutate,msg", [
    ("whole_plane", "window wider than the tap set"),
    ("tight", "window misses a pixel with a live tap"),
])
def test_yolact_window_mutants_fail_the_bounds(mutate, msg):
    case = sc.yolact_case(*sc.YOLACT_SHAPES[0])
    dense, _ = sc.yolact_dense(ora, case)
    planes, wins = sc.model_yolact(case, dense, _poisoned(dense.shape), np.full(dense.shape[:2] + (4,), sc.WIN_POISON, np.int32), mutate)
    with pytest.raises(AssertionError, match=msg):
        sc.check_yolact_window_bounds(case, wins)


@pytest.mark.parametrize("mutate,checker,msg", [
    ("window_short_row", "containment", "set pixel outside the reported window"),
    ("window_short_row", "chain", "through the window"),
    ("skip_last_row", "coverage", "byte inside the window differs"),
    ("skip_last_row", "chain", "through the window"),
])
def test_yolact_mutants_fail_their_checker(mutate, checker, msg):
    case = sc.yolact_case(*sc.YOLACT_SHAPES[0])
    dense, _ = sc.yolact_dense(ora, case)
    planes, wins = sc.model_yolact(case, dense, _poisoned(dense.shape), np.full(dense.shape[:2] + (4,), sc.WIN_POISON, np.int32), mutate)
    with pytest.raises(AssertionError, match=msg):
        if checker == "containment": sc.check_containment(dense, wins, case["counts"], case["names"])
        if checker == "coverage": sc.check_coverage(planes, dense, wins, case["counts"], case["names"])
        if checker == "chain": sc.check_chain(sc.windowed_encoder(ora), ora, planes, case["counts"], wins, dense, sc.image_sizes(case))


# ------------------------------------------------------------------------------------------------------------------ mask-IoU net reference
def test_fmaf_is_the_single_rounding_of_the_exact_value():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(np.float32); b = rng.standard_normal(400).astype(np.float32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-9, 3, 400)).astype(np.float32)
    # double-rounding traps: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies exactly half an fp32 ulp above a representable value; a residue far below
    # fp64's last bit decides the direction (a sum rounded to fp64 first loses it and ties to even)
    a = np.concatenate([a, np.full(5, 1 + 2.0 ** -12, np.float32)]); b = np.concatenate([b, np.full(5, 1 + 2.0 ** -12, np.float32)])
    c = np.concatenate([c, np.array([0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -80, -2.0 ** -100], np.float32)])
    got = sc.fmaf(a, b, c)
    assert got[-4] > got[-3]
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact)) if abs(exact) < 1e30 else None     # float(Fraction) rounds once to fp64: only a bracket here
        lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
        best = min((lo, near, hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


def test_maskiou_conv1_reference_is_within_its_fp64_bound():
    rng = np.random.default_rng(4)
    lo = rng.uniform(0, 1, (5, 9, 8)).astype(np.float32) * (rng.uniform(0, 1, (5, 9, 8)) < 0.7)
    w = rng.standard_normal((8, 9)).astype(np.float32); b = rng.standard_normal(8).astype(np.float32)
    got, exact, mag = sc.maskiou_conv1_ref(lo, w, b)
    u = 2.0 ** -24
    assert got.shape == (5, 4, 3, 8) and (got > 0).any() and (got == 0).any()
    assert (np.abs(got.astype(np.float64) - np.maximum(exact, 0)) <= 11 * u / (1 - 11 * u) * mag).all()


# ------------------------------------------------------------------------------------------------------------------ the new entry points
def test_new_entries_refuse_null_and_sizes_before_any_launch():
    """made-up device addresses that nothing dereferences: every refused call returns before its launch"""
    from isegmi import _ffi
    lib, fake = _ffi.lib(), 0x10000
    assert lib.isegmi_op_paste_masks_win(fake, fake, fake, 1, 1, 28, 4, 4, 0.5, None, None, 0, None) != 0
    assert b"paste_masks_win: null pointer" in lib.isegmi_last_error()
    assert lib.isegmi_op_paste_masks_win(fake, fake, fake, 1, 0, 28, 4, 4, 0.5, fake, None, 0, None) != 0
    assert b"paste_masks_win sizes" in lib.isegmi_last_error()
    assert lib.isegmi_op_yolact_masks_win(fake, fake, fake, fake, 1, 9, 8, 32, 4, 5, 5, None, fake, None, None, None, 0, 0, None) != 0
    assert b"yolact_masks_win: null pointer" in lib.isegmi_last_error()
    assert lib.isegmi_op_yolact_masks_win(fake, fake, fake, fake, 1, 9, 8, 31, 4, 5, 5, fake, fake, None, None, None, 0, 0, None) != 0
    assert b"mask_dim must be 32" in lib.isegmi_last_error()
    assert lib.isegmi_op_yolact_masks_win(fake, fake, fake, fake, 1, 9, 8, 32, 4, 1 << 16, 1 << 15, fake, fake, None, None, None, 0, 0, None) != 0
    assert b"below 2^31" in lib.isegmi_last_error()
    assert lib.isegmi_op_maskiou_conv1(fake, 1, 3, 3, fake, None, fake, None) != 0
    assert b"maskiou_conv1: null pointer" in lib.isegmi_last_error()
    assert lib.isegmi_op_maskiou_conv1(fake, 1, 2, 3, fake, fake, fake, None) != 0
    assert b"maskiou_conv1 sizes" in lib.isegmi_last_error()
    assert lib.isegmi_op_maskiou_rescore(fake, 1, 1, 1, 1, fake, fake, None, fake, None) != 0
    assert b"maskiou_rescore: null pointer" in lib.isegmi_last_error()
    assert lib.isegmi_op_maskiou_rescore(fake, 1, 1, 0, 1, fake, fake, fake, fake, None) != 0
    assert b"maskiou_rescore sizes" in lib.isegmi_last_error()
