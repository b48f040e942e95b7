"""No GPU: the CPU oracle against the plain references of tests/spatial_ref.py at every shape and input tests/test_spatial_f16_gpu.py and
tests/test_spatial_gpu.py hand to the kernels -- exact where the reference is exact, inside the derived bound elsewhere.  This is what shows that the
references and the bounds are sound before a kernel is compared with them: a bound the oracle alone does not meet is a wrong derivation."""
import numpy as np
import pytest

import spatial_cases as sc
import spatial_ref as ref
from oracle import ora


def f32(x):
    return np.asarray(x).astype(np.float32)


# ---------------------------------------------------------------- max-pool
def _maxpool_pair(shape, ksp, dt, key):
    x = sc.maxpool_input(shape, dt, True, key)
    a = ora.maxpool(f32(x), *ksp)
    b = ref.maxpool(x, *ksp)
    assert sc.same_bits(sc.h(a), sc.h(b)), (shape, ksp)
    if dt == np.float32:
        assert sc.same_bits(a, b), (shape, ksp)
    assert a.shape[1:3] == sc.maxpool_out_hw(shape[1], shape[2], *ksp)
    return sc.h(ora.maxpool(f32(sc.maxpool_input(shape, dt, False, key)), *ksp))


@pytest.mark.parametrize("form,in_f16,C", sc.MAXPOOL_F16_FORMS)
def test_maxpool_oracle_is_the_index_reference_f16_cases(form, in_f16, C):
    zeros = set()
    for shape, ksp in sc.maxpool_cases_small(C):
        dirty = _maxpool_pair(shape, ksp, np.float16 if in_f16 else np.float32, form)
        assert not np.isnan(dirty).any()               # `>` never takes a NaN
        zeros |= set(sc.bits(dirty)[dirty == 0].tolist())
    assert zeros == {0x0000, 0x8000}                    # the inputs do make windows whose maximum is a zero of either sign


@pytest.mark.parametrize("C", sc.MAXPOOL_F32_C)
def test_maxpool_oracle_is_the_index_reference_f32_cases(C):
    for shape, ksp in sc.maxpool_cases_small(C):
        _maxpool_pair(shape, ksp, np.float32, "f32")


def test_maxpool_oracle_is_the_index_reference_large_cases():
    for shape, ksp in sc.MAXPOOL_MODEL:
        _maxpool_pair(shape, ksp, np.float16, "model")
    _maxpool_pair(*sc.MAXPOOL_GRID_STRIDE, np.float16, "grid")
    _maxpool_pair(*sc.MAXPOOL_GRID_STRIDE, np.float32, "grid")
    shape, ksp = sc.MAXPOOL_GRID_STRIDE
    ho, wo = sc.maxpool_out_hw(shape[1], shape[2], *ksp)
    items = shape[0] * ho * wo * shape[3] // 8
    assert items > 4096 * 256 and items % (4096 * 256)


def test_maxpool_empty_outputs_are_left_out():
    assert sc.maxpool_out_hw(1, 9, 2, 2, 0) == (0, 0) and ref.maxpool_out_hw(1, 9, 2, 2, 0) == (0, 0)
    kept = list(sc.maxpool_cases_small(8))
    assert ((2, 1, 9, 8), (2, 2, 0)) not in kept and ((2, 1, 9, 8), (3, 2, 1)) in kept and len(kept) >= 25


# ---------------------------------------------------------------- nearest 2x + add
@pytest.mark.parametrize("dt,Cs", [(np.float16, sc.NEAREST_C), (np.float32, sc.NEAREST_F32_C)])
def test_nearest2x_add_oracle_is_the_index_reference(dt, Cs):
    seen_inf = seen_zero = inexact = 0
    for C in Cs:
        for N in sc.NEAREST_N:
            for Hc, Wc, H, W in sc.nearest_geometries():
                coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, dt)
                a = ora.upsample_nearest2x_add(f32(coarse), f32(lat))
                b = ref.nearest2x_add(f32(coarse), f32(lat))
                assert sc.same_bits(a, b) and not np.isnan(a).any(), (C, N, Hc, Wc, H, W)
                out = a.astype(dt) if dt == np.float32 else sc.h(a)
                seen_inf += int(np.isinf(out).sum()); seen_zero += int((out == 0).sum())
                inexact += int((out.astype(np.float64) != coarse_up(coarse, H, W).astype(np.float64) + lat.astype(np.float64)).sum())
    assert seen_inf > 100 and seen_zero > 100 and inexact > 1000       # overflow, cancellation and rounding all occur


def coarse_up(coarse, H, W):
    yi = np.minimum(np.arange(H) >> 1, coarse.shape[1] - 1); xi = np.minimum(np.arange(W) >> 1, coarse.shape[2] - 1)
    return coarse[:, yi][:, :, xi]


def test_nearest2x_add_large_case():
    N, Hc, Wc, C, H, W = sc.NEAREST_GRID_STRIDE
    for dt in (np.float16, np.float32):
        coarse, lat = sc.nearest_input(N, Hc, Wc, C, H, W, dt, "grid")
        assert sc.same_bits(ora.upsample_nearest2x_add(f32(coarse), f32(lat)), ref.nearest2x_add(f32(coarse), f32(lat)))
    assert N * H * W * C // 4 > 4096 * 256 and (N * H * W * C // 4) % (4096 * 256)


# ---------------------------------------------------------------- bilinear resize
def _resize_within_bound(case, dt, key=0, combos=((False, 0), (False, 1), (True, 0), (True, 1))):
    N, H, W, C, Ho, Wo = case
    x, add = sc.resize_input(case, dt, key)
    for use_add, relu in combos:
        a = add if use_add else None
        got = ora.resize_bilinear(f32(x), Ho, Wo, None if a is None else f32(a), relu)
        r64, bound = ref.resize_bilinear(x, Ho, Wo, a, relu)
        err = np.abs(got.astype(np.float64) - r64)
        assert (err <= bound).all(), (case, use_add, relu, float((err - bound).max()))
        if dt == np.float16:
            err = np.abs(sc.h(got).astype(np.float64) - r64)
            assert (err <= bound + ref.f16_store_slack(r64, bound)).all(), (case, use_add, relu)
        if (H, W) == (Ho, Wo) and not use_add and not relu:
            assert sc.same_bits(got, f32(x))            # identity: src = dst exactly, the far taps weigh 0


@pytest.mark.parametrize("case", sc.RESIZE_F32_CASES)
def test_resize_oracle_within_derived_bound_f32(case):
    _resize_within_bound(case, np.float32)


@pytest.mark.parametrize("case", sc.RESIZE_CASES)
def test_resize_oracle_within_derived_bound_f16(case):
    _resize_within_bound(case, np.float16)


def test_resize_large_case_within_derived_bound():
    for dt in (np.float16, np.float32):
        _resize_within_bound(sc.RESIZE_GRID_STRIDE, dt, "grid", ((True, 1),))


def test_resize_reference_against_torch():
    """The fp64 reference is F.interpolate(bilinear, align_corners=False) (a second opinion on the formula, in fp64 on both sides)."""
    torch = pytest.importorskip("torch")
    for case in [(2, 20, 30, 32, 7, 11), (1, 18, 18, 256, 35, 35), (2, 1, 1, 4, 5, 6), (3, 5, 1, 4, 3, 8)]:
        x, _ = sc.resize_input(case, np.float32)
        t = torch.nn.functional.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), (case[4], case[5]), mode="bilinear",
                                            align_corners=False).permute(0, 2, 3, 1).numpy()
        r64, _ = ref.resize_bilinear(x, case[4], case[5])
        assert np.abs(t - r64).max() < 1e-12 * max(1.0, np.abs(x).max())


# ---------------------------------------------------------------- avgpool_full
@pytest.mark.parametrize("shape", sc.AVGPOOL_CASES)
def test_avgpool_oracle_within_derived_bound(shape):
    x = (sc.rng_for("avgpool", shape).standard_normal(shape) * 2.0 + 0.5).astype(np.float32)
    mean, bound = ref.avgpool_full(x)
    err = np.abs(ora.avgpool_full(x).astype(np.float64) - mean)
    assert (err <= bound).all(), float((err - bound).max())


# ---------------------------------------------------------------- mask tail
def _ora_mask(feat, w, b, labels, rows=64):
    out = np.empty(feat.shape[:2], np.float32)
    for r0 in range(0, feat.shape[0], rows):
        out[r0:r0 + rows] = ora.mask_logits_select(f32(feat[r0:r0 + rows]), w, b, np.maximum(labels[r0:r0 + rows], 1))
    return out


def _chain_within_bound(R, HW, C, dt, labels):
    w, b = sc.mask_weights(C)
    feat = sc.mask_feat(R, HW, C, dt)
    got = _ora_mask(feat, w, b, labels)
    r64, bound = ref.mask_logits_select(feat, w, b, labels, depth=C + 1)
    on = labels >= 1
    err = np.abs(got.astype(np.float64) - r64)[on]
    assert (err <= bound[on]).all(), (R, HW, C, float((err - bound[on]).max()))
    assert not r64[~on].any() and not bound[~on].any()
    return feat, w, b, r64, on


@pytest.mark.parametrize("C", sc.MASK_GENERIC_C)
def test_mask_chain_within_derived_bound_f16_cases(C):
    for HW in sc.MASK_GENERIC_HW:
        _chain_within_bound(11, HW, C, np.float16, sc.mask_labels(11, sc.rng_for("mask_lab", C, HW), True))


@pytest.mark.parametrize("C", sc.MASK_F32_C)
def test_mask_chain_within_derived_bound_f32_cases(C):
    for HW in sc.MASK_F32_HW:
        _chain_within_bound(9, HW, C, np.float32, sc.mask_labels(9, sc.rng_for("mask_lab32", C, HW), True))


@pytest.mark.parametrize("R", sc.MASK_C256_R)
def test_mask_c256_association_within_derived_bound(R):
    """The kernel's own order (8 chained FMAs per lane, pairwise over 32 lanes, the bias), restated in numpy fp32, stays inside the depth-14 bound
    of the fp64 reference at every case of the GPU test; so does the oracle's 257-deep chain inside its own."""
    for HW in sc.MASK_C256_HW:
        labels = sc.mask_labels(R, sc.rng_for("mask_lab", 256, HW, R), True)
        feat, w, b, _, on = _chain_within_bound(R, HW, 256, np.float16, labels)
        z = sc.mask_c256_kernel_association(feat, w, b, labels)
        r64, bound = ref.mask_logits_select(feat, w, b, labels, depth=14)
        err = np.abs(ora.map_f32(z[on], 1).astype(np.float64) - r64[on])
        assert (err <= bound[on]).all(), (R, HW, float((err - bound[on]).max()))
        assert bound[on].max() < 1e-5                   # 14u x sum |x w| / 4, sum |x w| ~ 15 here: a dropped channel or pixel is far outside it


# ---------------------------------------------------------------- grid_anchors, pad_c3_to_c4
def test_grid_anchors_reference_is_the_host_generator():
    from isegmi.maskrcnn import grid_anchors
    for A in sc.ANCHOR_A:
        for stride in sc.ANCHOR_STRIDES:
            base = sc.anchor_base(A, stride)
            for gh, gw in sc.ANCHOR_GRIDS:
                a = ref.grid_anchors(base, stride, gh, gw)
                assert a.shape == (gh * gw * A, 4) and sc.same_bits(a, grid_anchors(gh, gw, stride, base)), (A, stride, gh, gw)
                assert sc.same_bits(a[(gw * (gh - 1) + gw - 1) * A:], base + np.float32(stride) * np.array([gw - 1, gh - 1, gw - 1, gh - 1], np.float32))


def test_pad_reference():
    x = np.arange(15, dtype=np.float32).reshape(5, 3) - 7
    p = ref.pad_c3_to_c4(x)
    assert p.shape == (5, 4) and np.array_equal(p[:, :3], x) and (sc.bits(p[:, 3]) == 0).all()
