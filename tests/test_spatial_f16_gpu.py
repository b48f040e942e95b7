"""The fp16 spatial kernels of csrc/spatial_f16.hip, operator by operator.  Their contract (the file's header): all arithmetic is fp32 in the order of the
fp32 kernels / the oracle, only loads and stores convert -- so fp16(ora.<op>(fp32(x))) is an exact reference for every one of them except the C = 256
mask tail, whose butterfly is held to the derived bound of tests/spatial_ref.py.  Every comparison is on the raw bits unless a bound is named.  The
same shapes and inputs are run oracle-against-reference, without a GPU, by tests/test_spatial_ref_cpu.py."""
import gc

import numpy as np
import pytest

import spatial_cases as sc
import spatial_ref as ref
from oracle import ora

pytestmark = pytest.mark.gpu

F16_CAP = 4096 * 256        # the grid cap of spatial_f16.hip's launchers, in work items


def f32(x):
    return np.asarray(x).astype(np.float32)


def no_sentinel(got):
    """The wrappers fill the output with 0xFF bytes: an fp16 / fp32 element nobody wrote reads back as that NaN pattern."""
    b = sc.bits(got)
    return not (b == np.array(-1).astype(b.dtype)).any()


# ---------------------------------------------------------------- max-pool: c8, half_t quad and float forms
def _check_maxpool(ffi, shape, ksp, in_f16, key):
    dt = np.float16 if in_f16 else np.float32
    for clean in (False, True):
        x = sc.maxpool_input(shape, dt, clean, key)
        got = ffi.maxpool_f16(x, *ksp, in_f16=in_f16)
        want = sc.h(ora.maxpool(f32(x), *ksp))
        assert got.dtype == np.float16 and sc.same_bits(got, want), (shape, ksp, clean, int((sc.bits(got) != sc.bits(want)).sum()))
        if clean:
            assert sc.same_bits(got, sc.h(ref.maxpool(x, *ksp))), (shape, ksp)


@pytest.mark.parametrize("form,in_f16,C", sc.MAXPOOL_F16_FORMS)
def test_maxpool_f16_sweep(ffi, form, in_f16, C):
    """+-inf, NaN, +-0 side by side (the `>` keeps the first seen: the zero's sign is part of the answer), 65504, subnormals and, for the float
    form, values the store rounds; every (k, s, p) and map size whose output is not empty."""
    n = 0
    for shape, ksp in sc.maxpool_cases_small(C):
        _check_maxpool(ffi, shape, ksp, in_f16, form)
        n += 1
    assert n >= 25


@pytest.mark.parametrize("shape,ksp", sc.MAXPOOL_MODEL)
def test_maxpool_f16_model_shapes(ffi, shape, ksp):
    _check_maxpool(ffi, shape, ksp, True, "model")
    gc.collect()


def test_maxpool_f16_rejects_what_it_cannot_take(ffi):
    x = np.zeros((1, 4, 4, 6), np.float16)
    with pytest.raises(ffi.IsegmiError):
        ffi.maxpool_f16(x, 3, 2, 1)                      # C % 4
    with pytest.raises(ffi.IsegmiError):
        ffi.maxpool_f16(np.zeros((1, 1, 5, 8), np.float16), 2, 2, 0)     # empty output
    with pytest.raises(ffi.IsegmiError):
        ffi.resize_bilinear_f16(x, 8, 8)
    with pytest.raises(ffi.IsegmiError):
        ffi.upsample_nearest2x_add_f16(x, np.zeros((1, 8, 8, 6), np.float16))
    with pytest.raises(ffi.IsegmiError):
        ffi.mask_logits_select_f16(np.zeros((2, 5, 6), np.float16), np.zeros((3, 6)), np.zeros(3), np.ones(2))


# ---------------------------------------------------------------- nearest 2x + add
@pytest.mark.parametrize("N", sc.NEAREST_N)
@pytest.mark.parametrize("C", sc.NEAREST_C)
def test_nearest2x_add_f16_sweep(ffi, C, N):
    for Hc, Wc, H, W in sc.nearest_geometries():
        coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, np.float16)
        got = ffi.upsample_nearest2x_add_f16(coarse, lat)
        want = sc.h(ora.upsample_nearest2x_add(f32(coarse), f32(lat)))
        assert sc.same_bits(got, want), (Hc, Wc, H, W)
        assert sc.same_bits(got, sc.h(ref.nearest2x_add(f32(coarse), f32(lat)))), (Hc, Wc, H, W)


# ---------------------------------------------------------------- bilinear resize
@pytest.mark.parametrize("case", sc.RESIZE_CASES)
def test_resize_bilinear_f16(ffi, case):
    N, H, W, C, Ho, Wo = case
    x, add = sc.resize_input(case, np.float16)
    for use_add in (False, True):
        for relu in (0, 1):
            a = add if use_add else None
            got = ffi.resize_bilinear_f16(x, Ho, Wo, a, relu)
            want = sc.h(ora.resize_bilinear(f32(x), Ho, Wo, None if a is None else f32(a), relu))
            assert sc.same_bits(got, want), (case, use_add, relu)
            r64, bound = ref.resize_bilinear(x, Ho, Wo, a, relu)
            err = np.abs(got.astype(np.float64) - r64)
            tol = bound + ref.f16_store_slack(r64, bound)
            assert (err <= tol).all(), (case, use_add, relu, float((err - tol).max()))


# ---------------------------------------------------------------- mask tail
def _ora_mask(feat, w, b, labels):
    """the oracle indexes w[label] whatever the label: rows with label <= 0 are evaluated with label 1 and not compared"""
    return ora.mask_logits_select(f32(feat), w, b, np.maximum(labels, 1))


def _check_empty_rows(got, labels):
    off = labels <= 0
    assert no_sentinel(got) and not np.isnan(got).any()
    assert (sc.bits(got[off]) == 0).all()                 # exactly +0.0


@pytest.mark.parametrize("HW", sc.MASK_GENERIC_HW)
@pytest.mark.parametrize("C", sc.MASK_GENERIC_C)
def test_mask_tail_f16_generic_exact(ffi, C, HW):
    """C != 256: one FMA chain in channel order on both sides."""
    R = 11
    labels = sc.mask_labels(R, sc.rng_for("mask_lab", C, HW), True)
    assert (labels == 0).any() and (labels == -1).any()
    w, b = sc.mask_weights(C)
    feat = sc.mask_feat(R, HW, C, np.float16)
    got = ffi.mask_logits_select_f16(feat, w, b, labels)
    want = _ora_mask(feat, w, b, labels)
    on = labels >= 1
    assert sc.same_bits(got[on], want[on])
    _check_empty_rows(got, labels)


@pytest.mark.parametrize("R", sc.MASK_C256_R)
@pytest.mark.parametrize("HW", sc.MASK_C256_HW)
def test_mask_tail_f16_c256_within_bound(ffi, HW, R):
    """Every residue the q0 += 32 walk, the two half-waves and the four pixels in flight can end on; pixel by pixel inside
    0.25 gamma(14) (sum |x w| + |b|) + 1.5e-7 of the fp64 reference."""
    labels = sc.mask_labels(R, sc.rng_for("mask_lab", 256, HW, R), True)
    w, b = sc.mask_weights(256)
    feat = sc.mask_feat(R, HW, 256, np.float16)
    got = ffi.mask_logits_select_f16(feat, w, b, labels)
    r64, bound = ref.mask_logits_select(feat, w, b, labels, depth=14)
    err = np.abs(got.astype(np.float64) - r64)
    assert got.shape == (R, HW) and (err <= bound).all(), (float((err - bound).max()), np.argwhere(err > bound)[:5].tolist())
    _check_empty_rows(got, labels)
    del feat, got, r64, bound, err
    gc.collect()


@pytest.mark.parametrize("HW", sc.MASK_C256_HW)
def test_mask_tail_f16_c256_same_bits_at_every_position(ffi, HW):
    """One pixel vector per row, placed at every position of the row: the butterfly must give the same bits whichever wave, half-wave and slot
    a pixel lands on (a lane- or slot-dependent error shows here even inside the bound)."""
    R = 37
    labels = sc.mask_labels(R, sc.rng_for("mask_lab_stable", HW), True)
    w, b = sc.mask_weights(256)
    pix = sc.mask_feat(R, 1, 256, np.float16, key="stable")
    feat = np.ascontiguousarray(np.broadcast_to(pix, (R, HW, 256)))
    got = ffi.mask_logits_select_f16(feat, w, b, labels)
    assert (sc.bits(got) == sc.bits(got)[:, :1]).all()
    one = ffi.mask_logits_select_f16(pix, w, b, labels)           # and they are the bits of the row that holds that pixel alone
    assert (sc.bits(got) == sc.bits(one)).all()
    _check_empty_rows(got, labels)


# ---------------------------------------------------------------- the grid-stride loop's second trip
def _tail_equal(got, want, items, per_item):
    lo, hi = sc.grid_stride_tail(items, per_item, F16_CAP)
    g, w_ = sc.bits(got).reshape(-1), sc.bits(want).reshape(-1)
    assert hi == g.size and lo < hi
    return np.array_equal(g[lo:hi], w_[lo:hi]) and np.array_equal(g[-per_item:], w_[-per_item:])


def test_maxpool_f16_grid_stride(ffi):
    shape, ksp = sc.MAXPOOL_GRID_STRIDE
    x = sc.maxpool_input(shape, np.float16, False, "grid")
    got = ffi.maxpool_f16(x, *ksp)
    want = sc.h(ora.maxpool(f32(x), *ksp))
    assert _tail_equal(got, want, got.size // 8, 8)
    assert sc.same_bits(got, want)
    del x, got, want
    gc.collect()


def test_nearest2x_add_f16_grid_stride(ffi):
    N, Hc, Wc, C, H, W = sc.NEAREST_GRID_STRIDE
    coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, np.float16, "grid")
    got = ffi.upsample_nearest2x_add_f16(coarse, lat)
    want = sc.h(ora.upsample_nearest2x_add(f32(coarse), f32(lat)))
    assert _tail_equal(got, want, got.size // 4, 4)
    assert sc.same_bits(got, want) and sc.same_bits(got, sc.h(ref.nearest2x_add(f32(coarse), f32(lat))))
    del coarse, lat, got, want
    gc.collect()


def test_resize_bilinear_f16_grid_stride(ffi):
    case = sc.RESIZE_GRID_STRIDE
    x, add = sc.resize_input(case, np.float16, "grid")
    got = ffi.resize_bilinear_f16(x, case[4], case[5], add, 1)
    want = sc.h(ora.resize_bilinear(f32(x), case[4], case[5], f32(add), 1))
    assert _tail_equal(got, want, got.size // 4, 4)
    assert sc.same_bits(got, want)
    del x, add, got, want
    gc.collect()
