"""RoIAlign and the LevelMapper AT their discrete decisions, every HIP form against an exact float64 answer and against the CPU oracle.  The inputs come from
tests/roi_align_cases.py; tests/test_roi_align_cases_cpu.py proves on the CPU that they sit on the edges they claim, that a naive reading of each edge
(`v <= -1`, `v >= size`, no clamp) gets them wrong, and that the oracle agrees with two independent statements of the operator.

Assertions, per form and family:
  (a) exact rows (integer features, power-of-two scales and bins): the float64 value bit for bit -- rounded to fp16 for the fp16 forms --, whatever the
      summation order; fixed grid 2 and the adaptive grid only (a 3 x 3 grid divides by 3)
  (b) everything: equal to the oracle, element for element; rows past counts[n] are +0 (the wrappers pre-fill the output with NaN)
  (c) everything: |got - ref| <= (gh gw + 9) 2^-24 S / (gh gw), S = sum |w| |v| (roi_align_cases.rounding_bound: derived, not measured); the fp16 forms add
      2^-11 |ref| + 2^-25
  (d) the level: out_level (plain fp32 forms) and the last entry of roi_prep's table equal the oracle's level, and level_f64 outside LEVEL_BAND; for the forms
      that report no level the "levels" family's maps hold (level index + 1), so (b) and (c) fail on a wrong level

Which form reaches what (FORMS below; every family x PH in {7, 14} x aligned in {0, 1} goes through every form that accepts it):
  f32_s2        roi_align_kernel<2>                              ffi.roi_align, sampling 2, C = 64
  f32_s0        roi_align_kernel<0>, adaptive grid               ffi.roi_align, sampling 0 (also the only form the "adaptive" family takes: ceilf of the bin
                                                                 size at 2, one ulp above 2, 1, 1/2; gh != gw; the empty grids of aligned boxes with x2 <= x1 or
                                                                 y2 <= y1, which pool to +0 since count = max(gh * gw, 1))
  f32_g3        roi_align_kernel<0>, run-time g = 3              ffi.roi_align, sampling 3
  tab_f32_row   roi_prep_kernel + roi_align_tab_kernel<7,7> / <14,14>, rows in index order      ffi.roi_prep + ffi.roi_align_ordered(order=None)
  tab_f32_ord   the same under roi_prep's (level, Morton) order
  tab_f16_row   roi_prep_kernel (2-byte elements) + roi_align_f16_tab_kernel<7,7> / <14,14>, index order
  tab_f16_ord   the same under roi_prep's order
  f16_c8_s2     roi_align_f16_c8_kernel, g == 2 branch           ffi.roi_align_f16, C = 64
  f16_c8_g3     roi_align_f16_c8_kernel, run-time-g branch       ffi.roi_align_f16, sampling 3, C = 64
  f16_gen_s2    roi_align_f16_kernel (256 % (C / 8) != 0)        ffi.roi_align_f16, C = 48
  test_launch_shapes: N K = 1 (slices == max_slices), N K = 2100 (one slice per RoI), C = 36 at 7 x 7 (per = 441 over 2 slices; the generic fp16 kernel),
  C = 48 (generic fp16), C = 32 / 64 / 256 (ns = 1 / 2 / 8 of roi_align_tab_kernel, 1 / 4 of the fp16 one), counts 0, 1 and K in one batch
  `k >= counts[n]`: every Case pads its last image (and test_launch_shapes has counts of 0 and 1); `v < -1 || v > size`, the clamps at 0 and size - 1,
  H == 1 and W == 1 maps: exact_A / exact_B / exact_C and ulp_neighbours; the `> 1` minimum size: small_and_odd; floorf of the level: levels, single_level

Worst |got - ref| / bound of (c) per form, over every family and launch shape (MI355X; exact rows contribute 0):
  f32_s2 0.237   f32_s0 0.347   f32_g3 0.265   tab_f32_row 0.237   tab_f32_ord 0.237   launch shapes: plain fp32 0.262, fp32 table (row, ord) 0.262
  f16_c8_s2 0.9971   f16_c8_g3 0.9945   f16_gen_s2 0.9937   tab_f16_row 0.9971   tab_f16_ord 0.9971   launch shapes: plain fp16 0.9977, fp16 table 0.9970
  (the fp16 figures are the final rounding to fp16: half an ulp is 2^-11 |ref| at a value just above a power of two; the fp32 part of the bound is unused)"""
import numpy as np
import pytest

import roi_align_cases as rc
from oracle import ora

pytestmark = pytest.mark.gpu
F16, F32, F64 = np.float16, np.float32, np.float64

# name -> (C, sampling grid, fp16, launch form)
FORMS = {
    "f32_s2": (64, 2, False, "plain"), "f32_s0": (64, 0, False, "plain"), "f32_g3": (64, 3, False, "plain"),
    "tab_f32_row": (64, 2, False, "row"), "tab_f32_ord": (64, 2, False, "ord"), "tab_f16_row": (64, 2, True, "row"), "tab_f16_ord": (64, 2, True, "ord"),
    "f16_c8_s2": (64, 2, True, "plain"), "f16_c8_g3": (64, 3, True, "plain"), "f16_gen_s2": (48, 2, True, "plain")}
FAMILIES = {
    "exact_A": lambda PH, al: rc.exact_cases(PH, al)[0], "exact_B": lambda PH, al: rc.exact_cases(PH, al)[1], "exact_C": lambda PH, al: rc.exact_cases(PH, al)[2],
    "ulp_neighbours": rc.ulp_neighbour_case, "small_and_odd": rc.small_roi_case,
    "levels": lambda PH, al: rc.level_case(PH), "single_level": lambda PH, al: rc.single_level_case(PH), "adaptive": rc.adaptive_case}
WORST = {}


def _launch(ffi, case, feats, Cc, g, f16, how):
    """-> (out [N, K, PH, PW, C], levels [N, K] or None)"""
    PH, PW, shape = case.PH, case.PW, (case.N, case.K, case.PH, case.PW, Cc)
    if how == "plain":
        if f16:
            return ffi.roi_align_f16(feats, case.scales, case.rois, case.counts, PH, PW, sampling=g, k_min=case.k_min, aligned=case.aligned).reshape(shape), None
        out, lv = ffi.roi_align(feats, case.scales, case.rois, case.counts, PH, PW, sampling=g, k_min=case.k_min, aligned=case.aligned)
        return out.reshape(shape), lv
    assert g == 2
    order, tab = ffi.roi_prep(case.rois, case.counts, case.shapes, case.scales, Cc, PH, PW, k_min=case.k_min, f16=f16, aligned=case.aligned)
    for n in range(case.N):   # roi_prep's order: a permutation of the image's rows, the rows inside counts[n] first
        assert sorted(order[n].tolist()) == list(range(n * case.K, (n + 1) * case.K)) and (order[n, :case.counts[n]] - n * case.K < case.counts[n]).all()
    out = ffi.roi_align_ordered(feats, case.scales, case.rois, case.counts, PH, PW, order if how == "ord" else None, tab, k_min=case.k_min, f16=f16)
    return out.reshape(shape), tab.reshape(case.N, case.K, -1, 4)[:, :, -1, 0] + case.k_min


def _truth(case, Cc, g):
    feats = rc.make_feats(case, Cc)
    out, levels = rc.run_oracle(ora, case, feats, g)
    ref, S, grids = rc.reference(case, feats, levels, g)
    return feats, out, levels, ref, rc.bound_of(S, grids)


def _check(name, tag, case, truth, got, levels, g, f16):
    _, out, lv_ora, ref, bound = truth
    valid = np.arange(case.K)[None, :] < case.counts[:, None]
    assert not got[~valid].view(np.uint16 if f16 else np.uint32).any(), (name, tag, "rows past counts are not +0")
    if levels is not None:                                                                                  # (d)
        lf, t = rc.level_f64(case.rois.reshape(-1, 4), case.k_min, case.k_max)
        sure = valid & ~rc.in_level_band(t).reshape(valid.shape)
        assert np.array_equal(levels[valid], lv_ora[valid]) and np.array_equal(levels[sure], lf.reshape(valid.shape)[sure]), (name, tag, "level")
    assert np.array_equal(got, out.astype(F16) if f16 else out), (name, tag, "differs from the oracle")      # (b)
    if g in (2, 0):                                                                                         # (a)
        m = case.exact_mask()
        want = ref[m].astype(F16) if f16 else ref[m]
        assert np.array_equal(got[m].astype(F64), want.astype(F64)), (name, tag, "an exact row is not the float64 value")
    bnd = rc.f16_bound(bound, ref) if f16 else bound                                                        # (c)
    err = np.abs(got.astype(F64) - ref)
    ratio = float(np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0).max())
    print("RATIO %-12s %-28s %.4f" % (name, tag, ratio))
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert (err <= bnd).all(), (name, tag, "worst |got - ref| / bound = %.3f" % ratio)


def _run_forms(ffi, case, forms, tag):
    truths = {}
    for name in forms:
        Cc, g, f16, how = FORMS[name]
        if (Cc, g) not in truths:
            truths[Cc, g] = _truth(case, Cc, g)
        got, levels = _launch(ffi, case, truths[Cc, g][0], Cc, g, f16, how)
        _check(name, tag, case, truths[Cc, g], got, levels, g, f16)


# (the level does not depend on `aligned`: the two level families run under aligned = 0 only)
@pytest.mark.parametrize("family,PH,aligned", [(f, PH, al) for f in FAMILIES for PH in (7, 14) for al in (0, 1)
                                               if f != "adaptive" and not (al and f in ("levels", "single_level"))])
def test_fixed_grid_families_through_every_form(ffi, family, PH, aligned):
    _run_forms(ffi, FAMILIES[family](PH, aligned), list(FORMS), "%s PH=%d aligned=%d" % (family, PH, aligned))


@pytest.mark.parametrize("aligned", [0, 1])
@pytest.mark.parametrize("PH", [7, 14])
def test_adaptive_grid_and_its_empty_grids(ffi, PH, aligned):
    """roi_align_kernel<0> with sampling 0 on the C4 geometry; under aligned = 1 the boxes with x2 <= x1 or y2 <= y1 have an empty grid and must give +0 (they
    gave 0 / 0 = NaN before count = max(gh * gw, 1)); under sampling 2 the same boxes have defined, exact values (exact_A carries them)."""
    case = rc.adaptive_case(PH, aligned)
    _run_forms(ffi, case, ["f32_s0"], "adaptive PH=%d aligned=%d" % (PH, aligned))
    feats = rc.make_feats(case, 64)
    out, _ = ffi.roi_align(feats, case.scales, case.rois, case.counts, PH, PH, sampling=0, k_min=4, aligned=aligned)
    empty = [row for row, _, _, grid, _, _ in case.tags if grid is not None and (grid[0] <= 0 or grid[1] <= 0)]
    assert len(empty) == (5 if aligned else 0)
    assert np.isfinite(out).all() and not out[empty].view(np.uint32).any()
    assert all(np.abs(f).max() == 8 for f in feats)                                   # (the maps are not zero)


LAUNCH_SHAPES = [   # (N, K, counts, C, PH)
    (1, 1, [1], 64, 7), (1, 1, [1], 64, 14), (3, 700, [700, 1, 0], 32, 7), (3, 64, [0, 1, 64], 36, 7), (3, 64, [0, 1, 64], 48, 7), (3, 64, [0, 1, 64], 32, 14),
    (3, 64, [0, 1, 64], 64, 7), (3, 64, [0, 1, 64], 256, 7), (2, 40, [40, 13], 256, 14)]


@pytest.mark.parametrize("N,K,counts,Cc,PH", LAUNCH_SHAPES)
def test_launch_shapes(ffi, N, K, counts, Cc, PH):
    case = rc.launch_case(N, K, counts, PH, seed=Cc + PH)
    truth = _truth(case, Cc, 2)
    assert len(set(truth[2][np.arange(K)[None, :] < case.counts[:, None]].tolist())) >= min(3, sum(counts))     # several levels in use
    forms = [("f32", False, "plain"), ("f16", True, "plain")]
    forms += [("tab_f32_" + h, False, h) for h in ("row", "ord") if Cc in (32, 64, 128, 256)] + [("tab_f16_" + h, True, h) for h in ("row", "ord") if Cc in (64, 128, 256)]
    for name, f16, how in forms:
        got, levels = _launch(ffi, case, truth[0], Cc, 2, f16, how)
        _check("launch_" + name, "N=%d K=%d C=%d PH=%d" % (N, K, Cc, PH), case, truth, got, levels, 2, f16)
