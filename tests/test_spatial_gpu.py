"""The fp32 spatial ops (csrc/spatial.hip) and the small R-CNN tails next to them through their operator entries, swept over the shapes and
values where such kernels go wrong: exact against the CPU oracle, and against the plain references of tests/spatial_ref.py (exact where those
are exact, inside the bound derived there elsewhere).  tests/test_spatial_ref_cpu.py runs oracle against reference at the same inputs."""
import gc

import numpy as np
import pytest

import spatial_cases as sc
import spatial_ref as ref
from oracle import ora

pytestmark = pytest.mark.gpu

F32_CAP = 2048 * 256        # the grid cap of spatial.hip's launchers, in work items


def no_sentinel(got):
    return not (sc.bits(got) == 0xFFFFFFFF).any()


def _check_maxpool(ffi, shape, ksp, key):
    for clean in (False, True):
        x = sc.maxpool_input(shape, np.float32, clean, key)
        got = ffi.maxpool(x, *ksp)
        assert sc.same_bits(got, ora.maxpool(x, *ksp)), (shape, ksp, clean)
        if clean:
            assert sc.same_bits(got, ref.maxpool(x, *ksp)), (shape, ksp)


@pytest.mark.parametrize("C", sc.MAXPOOL_F32_C)
def test_maxpool_sweep(ffi, C):
    n = 0
    for shape, ksp in sc.maxpool_cases_small(C):
        _check_maxpool(ffi, shape, ksp, "f32")
        n += 1
    assert n >= 25


@pytest.mark.parametrize("shape,ksp", sc.MAXPOOL_MODEL)
def test_maxpool_model_shapes(ffi, shape, ksp):
    _check_maxpool(ffi, shape, ksp, "model")
    gc.collect()


@pytest.mark.parametrize("N", sc.NEAREST_N)
@pytest.mark.parametrize("C", sc.NEAREST_F32_C)
def test_nearest2x_add_sweep(ffi, C, N):
    for Hc, Wc, H, W in sc.nearest_geometries():
        coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, np.float32)
        got = ffi.upsample_nearest2x_add(coarse, lat)
        assert sc.same_bits(got, ora.upsample_nearest2x_add(coarse, lat)), (Hc, Wc, H, W)
        assert sc.same_bits(got, ref.nearest2x_add(coarse, lat)), (Hc, Wc, H, W)


@pytest.mark.parametrize("case", sc.RESIZE_F32_CASES)
def test_resize_bilinear_sweep(ffi, case):
    N, H, W, C, Ho, Wo = case
    x, add = sc.resize_input(case, np.float32)
    for use_add in (False, True):
        for relu in (0, 1):
            a = add if use_add else None
            got = ffi.resize_bilinear(x, Ho, Wo, a, relu)
            assert sc.same_bits(got, ora.resize_bilinear(x, Ho, Wo, a, relu)), (case, use_add, relu)
            r64, bound = ref.resize_bilinear(x, Ho, Wo, a, relu)
            err = np.abs(got.astype(np.float64) - r64)
            assert (err <= bound).all(), (case, use_add, relu, float((err - bound).max()))


def _tail_equal(got, want, items, per_item):
    lo, hi = sc.grid_stride_tail(items, per_item, F32_CAP)
    g, w_ = sc.bits(got).reshape(-1), sc.bits(want).reshape(-1)
    assert hi == g.size and lo < hi
    return np.array_equal(g[lo:hi], w_[lo:hi]) and np.array_equal(g[-per_item:], w_[-per_item:])


def test_maxpool_grid_stride(ffi):
    shape, ksp = sc.MAXPOOL_GRID_STRIDE
    x = sc.maxpool_input(shape, np.float32, False, "grid")
    got = ffi.maxpool(x, *ksp)
    want = ora.maxpool(x, *ksp)
    assert _tail_equal(got, want, got.size // 4, 4) and sc.same_bits(got, want)
    del x, got, want
    gc.collect()


def test_nearest2x_add_grid_stride(ffi):
    N, Hc, Wc, C, H, W = sc.NEAREST_GRID_STRIDE
    coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, np.float32, "grid")
    got = ffi.upsample_nearest2x_add(coarse, lat)
    want = ora.upsample_nearest2x_add(coarse, lat)
    assert _tail_equal(got, want, got.size // 4, 4) and sc.same_bits(got, want) and sc.same_bits(got, ref.nearest2x_add(coarse, lat))
    del coarse, lat, got, want
    gc.collect()


def test_resize_bilinear_grid_stride(ffi):
    case = sc.RESIZE_GRID_STRIDE
    x, add = sc.resize_input(case, np.float32, "grid")
    got = ffi.resize_bilinear(x, case[4], case[5], add, 1)
    want = ora.resize_bilinear(x, case[4], case[5], add, 1)
    assert _tail_equal(got, want, got.size // 4, 4) and sc.same_bits(got, want)
    del x, add, got, want
    gc.collect()


@pytest.mark.parametrize("shape", sc.AVGPOOL_CASES)
def test_avgpool_full_sweep(ffi, shape):
    x = (sc.rng_for("avgpool", shape).standard_normal(shape) * 2.0 + 0.5).astype(np.float32)
    got = ffi.avgpool_full(x)
    assert sc.same_bits(got, ora.avgpool_full(x))
    mean, bound = ref.avgpool_full(x)
    err = np.abs(got.astype(np.float64) - mean)
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("HW", sc.MASK_F32_HW)
@pytest.mark.parametrize("C", sc.MASK_F32_C)
def test_mask_logits_select_sweep(ffi, C, HW):
    """Rows with label 0 and -1 are exactly +0.0 (the oracle indexes w[label] whatever the label, so it is the reference on the other rows only)."""
    R = 9
    labels = sc.mask_labels(R, sc.rng_for("mask_lab32", C, HW), True)
    assert (labels == 0).any() and (labels == -1).any()
    w, b = sc.mask_weights(C)
    feat = sc.mask_feat(R, HW, C, np.float32)
    got = ffi.mask_logits_select(feat, w, b, labels)
    on = labels >= 1
    want = ora.mask_logits_select(feat, w, b, np.maximum(labels, 1))
    assert sc.same_bits(got[on], want[on])
    assert no_sentinel(got) and not np.isnan(got).any() and (sc.bits(got[~on]) == 0).all()
    r64, bound = ref.mask_logits_select(feat, w, b, labels, depth=C + 1)
    err = np.abs(got.astype(np.float64) - r64)
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("A", sc.ANCHOR_A)
def test_grid_anchors_sweep(ffi, A):
    from isegmi.maskrcnn import grid_anchors
    for stride in sc.ANCHOR_STRIDES:
        base = sc.anchor_base(A, stride)
        for gh, gw in sc.ANCHOR_GRIDS:
            got = ffi.grid_anchors(base, stride, gh, gw)
            assert sc.same_bits(got, ref.grid_anchors(base, stride, gh, gw)), (A, stride, gh, gw)
            assert sc.same_bits(got, grid_anchors(gh, gw, stride, base)), (A, stride, gh, gw)


@pytest.mark.parametrize("npix", sc.PAD_NPIX)
def test_pad_c3_to_c4_sweep(ffi, npix):
    x = sc.rng_for("pad", npix).standard_normal((npix, 3)).astype(np.float32)
    got = ffi.pad_c3_to_c4(x)
    assert sc.same_bits(got, ref.pad_c3_to_c4(x))
    assert (sc.bits(got[-1]) == np.append(sc.bits(x[-1]), 0)).all()
