"""The inputs of tests/roi_align_cases.py discriminate (so that a green tests/test_roi_align_edges_gpu.py means something), and the oracle's RoIAlign and
LevelMapper -- fp32 restatements of the kernels -- get the second opinion they lacked: a float64 numpy statement of the operator and a torch.grid_sample one.

  exact cases      oracle == roi_align_f64 bit for bit under the grids that keep them exact (2 and adaptive); every value survives a float16 round trip
  tags             every tagged first / last sample sits on the coordinate it claims and falls on the side of `v < -1 || v > size` it claims
  naive variants   `v <= -1`, `v >= size` and "no clamp" each disagree with the reference on every edge they misread
  random RoIs      200 per setting: oracle vs roi_align_f64 under the derived rounding bound, vs grid_sample to 2e-6 on unit-variance features
  levels           oracle == level_f64 outside LEVEL_BAND, fewer than 5 % of a boundary's boxes inside it, both sides of every flip present
  zero grids       aligned, adaptive, x2 <= x1 or y2 <= y1: +0 everywhere (count = max(gh * gw, 1)), never NaN"""
import numpy as np
import pytest

import roi_align_cases as rc
from oracle import ora

F32, F64 = np.float32, np.float64
PHS, ALIGNED = [7, 14], [0, 1]
C_CPU = 8


def _truth(case, g, Cc=C_CPU):
    feats = rc.make_feats(case, Cc)
    out, levels = rc.run_oracle(ora, case, feats, g)
    ref, S, grids = rc.reference(case, feats, levels, g)
    return feats, out, levels, ref, rc.bound_of(S, grids), grids


def _within(got, ref, bound):
    err = np.abs(got.astype(F64) - ref)
    return bool((err <= bound).all())


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("PH", PHS)
def test_exact_cases_equal_the_float64_value_and_survive_fp16(PH, aligned):
    cases = rc.exact_cases(PH, aligned)
    assert [c.name for c in cases] == ["exact_A", "exact_B", "exact_C"] and all(c.exact for c in cases)
    for case, grids in [(c, (2, 0)) for c in cases] + [(rc.adaptive_case(PH, aligned), (0,))]:
        for g in grids:
            _, out, levels, ref, bound, _ = _truth(case, g)
            m = case.exact_mask()
            assert m.sum() >= 5 and np.array_equal(out[m].astype(F64), ref[m]), (case.name, g)
            assert np.array_equal(ref[m].astype(np.float16).astype(F64), ref[m]), (case.name, g)
            assert _within(out, ref, bound) and not np.isnan(out).any()
            assert not rc.in_level_band(rc.level_f64(case.rois.reshape(-1, 4))[1]).any()      # no level of these cases is in doubt
            lf = rc.level_f64(case.rois.reshape(-1, 4), case.k_min, case.k_max)[0].reshape(case.N, case.K)
            assert all(levels[n, k] == lf[n, k] for n, k in case.rows())
        if case.name == "exact_A":   # every level of the pyramid is in use
            assert sorted(set(int(levels[n, k]) for n, k in case.rows())) == [2, 3, 4, 5]


def _tag_samples(case, row, axis, g=2):
    n, k = divmod(row, case.K)
    assert k < case.counts[n]
    li = int(ora.level_map(case.rois[n, k:k + 1], case.k_min, case.k_max)[0]) - case.k_min
    ys, xs, *_ = rc.roi_geometry(case.rois[n, k], case.scales[li], case.PH, case.PW, g, case.aligned)
    H, W = case.shapes[li]
    return (ys, H) if axis == "y" else (xs, W)


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("PH", PHS)
def test_tagged_samples_sit_where_they_claim(PH, aligned):
    seen = set()
    for case in rc.exact_cases(PH, aligned) + [rc.ulp_neighbour_case(PH, aligned)]:
        for row, axis, which, coord, valid, label in case.tags:
            v, size = _tag_samples(case, row, axis)
            s = v[0, 0] if which == "first" else v[-1, -1]
            if coord is not None:
                assert s == F32(coord), (case.name, row, label, s)
                assert (not (s < -1 or s > size)) == valid
                seen.add((case.name, axis, "-1" if coord == -1 else "0" if coord == 0 else "size" if coord == size else "size-1" if coord == size - 1 else "in"))
            elif label == "wholly outside":
                assert ((v < -1) | (v > size)).all(), (case.name, row)
                seen.add((case.name, axis, "out-" + which))
            else:   # an ulp neighbour: just beyond, by less than 1e-5
                assert (-1 - 1e-5 < float(s) < -1) if which == "first" else (size < float(s) < size + 1e-5), (case.name, row, label, s)
                seen.add((case.name, axis, "ulp-" + which))
    for axis in "yx":
        assert {("exact_A", axis, e) for e in ("-1", "0", "size-1", "in", "size", "out-first", "out-last")} <= seen
        assert {("ulp_neighbours", axis, e) for e in ("ulp-first", "ulp-last", "-1", "size")} <= seen
        assert {(c, axis, e) for c in ("exact_B", "exact_C") for e in ("-1", "0", "size")} <= seen


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("PH", PHS)
def test_naive_readings_of_each_edge_disagree(PH, aligned):
    """`v <= -1` loses the sample at -1, `v >= size` the one at size, and without the clamps a sample in [-1, 0) or (size - 1, size] gives part of its weight
    to a tap outside the map.  Which variants must differ on a tagged RoI is read off its sample coordinates (any sample at -1, any at size, any valid one
    outside [0, size - 1]); each variant then differs on exactly those RoIs, the RoI tagged with the edge it misreads among them."""
    for case in rc.exact_cases(PH, aligned):
        feats = rc.make_feats(case, C_CPU)
        _, levels = rc.run_oracle(ora, case, feats, 2)
        ref = rc.reference(case, feats, levels, 2)[0].reshape(case.N * case.K, -1)
        diff = {v: (rc.reference(case, feats, levels, 2, variant=v)[0].reshape(case.N * case.K, -1) != ref).any(1) for v in ("lo_closed", "hi_closed", "no_clamp")}
        hits = {v: 0 for v in diff}
        for row, axis, which, coord, valid, label in case.tags:
            if coord is None:
                continue
            want = {v: False for v in diff}   # what the sample coordinates of both axes say each variant must get wrong
            for ax in "yx":
                v, size = _tag_samples(case, row, ax)
                ok = ~((v < -1) | (v > size))
                want["lo_closed"] |= bool((v == -1).any())
                want["hi_closed"] |= bool((v == size).any())
                want["no_clamp"] |= bool((ok & ((v < 0) | (v > size - 1))).any())
            size = _tag_samples(case, row, axis)[1]
            assert want["lo_closed"] or coord != -1
            assert want["hi_closed"] or coord != size
            assert want["no_clamp"] or not (valid and (coord < 0 or coord > size - 1))
            for v in diff:
                assert bool(diff[v][row]) == want[v], (case.name, row, label, coord, v)
                hits[v] += int(diff[v][row])
        assert all(h >= 2 for h in hits.values()), hits


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("PH", PHS)
def test_an_ulp_neighbours_lost_sample_is_2_to_the_20_bounds(PH, aligned):
    case = rc.ulp_neighbour_case(PH, aligned)
    assert len(case.tags) == 8
    _, out, _, ref, bound, _ = _truth(case, 2)
    assert _within(out, ref, bound)
    ref, bound = ref.reshape(-1, PH, PH, C_CPU), bound.reshape(ref.size // (PH * PH * C_CPU), PH, PH, C_CPU)
    for (row, axis, which, coord, _, _), (row2, *_) in zip(case.tags[0::2], case.tags[1::2]):
        assert coord is None and row2 == row + 1
        p = 0 if which == "first" else PH - 1
        a, b, bd = (t[row:row + 2, p] if axis == "y" else t[row:row + 2, :, p] for t in (ref, ref, bound))
        change = np.abs(a[0] - a[1])
        assert (change >= 2.0 ** 20 * bd[0]).all() and (change >= 2.0).all(), (row, axis, which, change.min())


@pytest.mark.parametrize("PH", PHS)
def test_small_rois_meet_the_minimum_size_only_when_not_aligned(PH):
    for aligned in ALIGNED:
        case = rc.small_roi_case(PH, aligned)
        sizes = [rc.roi_geometry(case.rois.reshape(-1, 4)[i], 0.25, PH, PH, 2, aligned)[4:] for i in range(4)]
        if aligned:
            assert sizes[0] == (F32(0.5), F32(0.25)) and sizes[1] == (F32(0.0625), F32(0.0625))
        else:
            assert sizes[0] == (1, 1) and sizes[1] == (1, 1)
        assert sizes[2] == (1, 1) and sizes[3][0] > 1 and sizes[3][1] > 1      # exactly one pixel: `> 1` or `>= 1`, the same value; an ulp above: kept
        for g in (2, 3, 0):
            _, out, _, ref, bound, _ = _truth(case, g)
            assert _within(out, ref, bound), (aligned, g)
    # the clamp matters: the same boxes under the two settings differ
    a, b = (_truth(rc.small_roi_case(PH, al), 2)[3] for al in ALIGNED)
    assert (a[0, 0] != b[0, 0]).any() and (a[0, 1] != b[0, 1]).any()


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("PH", PHS)
def test_adaptive_grids_are_the_tagged_ones_and_an_empty_grid_pools_to_plus_zero(PH, aligned):
    case = rc.adaptive_case(PH, aligned)
    _, out, _, ref, bound, grids = _truth(case, 0)
    assert _within(out, ref, bound)
    empty = 0
    for row, _, _, grid, _, label in case.tags:
        if grid is None:
            continue
        assert tuple(grids[0, row]) == grid, (label, grids[0, row])
        if grid[0] <= 0 or grid[1] <= 0:
            empty += 1
            assert not out[0, row].view(np.uint32).any() and not ref[0, row].any(), label     # +0 bits: not NaN, not -0
    assert empty == (5 if aligned else 0)
    assert np.isfinite(out).all()
    if aligned:   # under a fixed grid the same boxes have defined values (all of a bin's samples coincide along the flat axis), exact ones
        flat = rc.exact_cases(PH, 1)[0]
        _, o2, _, r2, _, _ = _truth(flat, 2)
        rows = o2.reshape(-1, PH, PH, C_CPU)[-4:]
        assert np.array_equal(rows.astype(F64), r2.reshape(-1, PH, PH, C_CPU)[-4:]) and rows.any(axis=(1, 2, 3)).all()


@pytest.mark.parametrize("aligned", ALIGNED)
@pytest.mark.parametrize("g", [2, 0])
def test_random_rois_oracle_against_float64_and_grid_sample(g, aligned):
    pytest.importorskip("torch")
    rng = np.random.default_rng(5 + 2 * g + aligned)
    H, W, Cc, n = 25, 42, 8, 200
    feat = rng.standard_normal((1, H, W, Cc)).astype(F32)
    rois = rc.random_boxes(rng, n, W * 16, H * 16, 8.0, 500.0)
    for PH in PHS:
        out = ora.roi_align(feat, np.concatenate([np.zeros((n, 1), F32), rois], 1), 1 / 16, PH, PH, g, aligned)
        worst = 0.0
        for i in range(n):
            ref, S, (gh, gw) = rc.roi_align_f64(feat[0], rois[i], 1 / 16, PH, PH, g, aligned)
            assert (np.abs(out[i] - ref) <= rc.rounding_bound(S, gh, gw)).all(), (PH, i)
            gs = rc.roi_align_grid_sample(feat[0], rois[i], 1 / 16, PH, PH, g, aligned)
            worst = max(worst, float(np.abs(out[i] - gs).max()), float(np.abs(ref - gs).max()))
        assert 0 < worst <= 2e-6, worst


def test_level_boundaries_oracle_against_float64_outside_a_thin_band():
    for side in rc.LEVEL_SIDES:
        boxes = rc.level_boxes(side)
        lf, t = rc.level_f64(boxes)
        band = rc.in_level_band(t)
        assert len(boxes) == 164 and 4 <= band.sum() < 0.05 * len(boxes), (side, band.sum(), len(boxes))
        lo = int(round(np.log2(side / 224.0))) + 3
        assert set(lf[~band]) == {lo, lo + 1} and set(lf[band]) == {lo, lo + 1}             # both sides of the flip, in the band too
        got = ora.level_map(boxes)
        assert np.array_equal(got[~band], lf[~band]), side
        assert set(got[band]) <= {lo, lo + 1}
        x2 = np.sort(boxes[:, 2])
        assert (np.diff(x2) == np.spacing(x2[:-1])).sum() >= 3                                 # the fp32 neighbours are there
    case = rc.level_case(7)
    far = case.rois[0, -4:]
    assert list(ora.level_map(far)) == [2, 2, 5, 5] == list(rc.level_f64(far)[0])
    t = rc.level_f64(far)[1]
    assert t[0] < 0 and t[1] < -3 and t[2] > 6 and t[3] > 10                                  # far outside [2, 5]: the clamp decides
    single = rc.single_level_case(7)
    flat = single.rois.reshape(-1, 4)
    assert (ora.level_map(flat, 4, 4) == 4).all() and (rc.level_f64(flat, 4, 4)[0] == 4).all()
    assert len(set(rc.level_f64(flat)[0])) >= 3                                               # ... where the four-level mapper would spread them
