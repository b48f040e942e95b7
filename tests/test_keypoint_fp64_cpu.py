"""The keypoint decode's fp64 reference and the inputs of tests/test_keypoint_edges_gpu.py, checked without a GPU: tests/keypoint_fp64.py
against torch in float64; the exact-input claim (the fp32 restatement tests/keypoint_ref.py equals fp64 elementwise on every case the GPU test runs); the
derived bound e on the thread-layout sweep and four altered restatements that must break it; and the case builders -- unique maxima where required, ties where
intended, every peak place hit, the non-finite expectations, the limits."""
import numpy as np

import keypoint_edge_cases as ke
import keypoint_fp64 as k64
import keypoint_ref as kr

F = np.float32


def test_fp64_reference_against_torch_and_at_the_identity():
    """torch's bicubic (A = -0.75, half-pixel centres, clamped taps) in float64: a differently written evaluation of the same definition."""
    import torch
    rng = np.random.default_rng(0)
    for s, hc, wc in ((56, 57, 113), (56, 7, 300), (64, 200, 3), (3, 5, 9), (1, 4, 2), (2, 1, 1)):
        m = rng.standard_normal((s, s))
        want = torch.nn.functional.interpolate(torch.from_numpy(m)[None, None], size=(hc, wc), mode="bicubic", align_corners=False)[0, 0].numpy()
        assert np.abs(k64.resize(m, hc, wc) - want).max() < 1e-13, (s, hc, wc)
    m = rng.standard_normal((56, 56))
    assert np.array_equal(k64.resize(m, 56, 56), m)
    R = k64.matrices(112, 56)[0]
    assert np.abs(R.sum(1) - 1.0).max() < 1e-15 and np.array_equal(np.nonzero(R[0])[0], [0, 1]) and np.array_equal(np.nonzero(R[-1])[0], [54, 55])
    box = (3.25, 2.75, 30.5, 17.25)
    for p in (0, 27, 28 * 15 - 1):
        assert k64.position_of(box, k64.keypoint(box, p)) == p


def test_exact_cases_restatement_equals_fp64():
    heat, boxes, count, cases, kpt, score, nmax = ke.exact_batch()
    assert count.tolist() == [29] and len(cases) == 29 and (56, 448, 100, False) in cases
    ratios = set()
    for i, (hc, wc, amp, ties) in enumerate(cases):
        w, h, wc_, hc_ = kr.box_sizes(boxes[0, i])
        assert (wc_, hc_) == (wc, hc) and boxes[0, i, 0] % 1 and boxes[0, i, 1] % 1
        ratios.add(float(w) / wc); ratios.add(float(h) / hc)
        assert np.abs(heat[i]).max() == amp and np.array_equal(heat[i], np.round(heat[i]))
        assert len({heat[i][:, :, k].tobytes() for k in range(17)}) == 17                     # all channels differ
        for k in range(17):
            r32 = kr.resize_bicubic(heat[i][:, :, k], hc, wc)
            assert np.array_equal(r32.astype(np.float64), k64.resize(heat[i][:, :, k], hc, wc)), (hc, wc, k)
        assert np.array_equal(score[i].astype(F).astype(np.float64), score[i])
        got_kpt, got_score, _ = kr.decode_one(heat[i], boxes[0, i])
        assert np.array_equal(got_kpt, kpt[i]) and np.array_equal(got_score.astype(np.float64), score[i])
        if ties:
            assert (nmax[i] >= 2).all(), (hc, wc, nmax[i])
        else:
            assert (nmax[i] == 1).all(), (hc, wc, nmax[i])
    assert len(ratios) >= 8 and 1.0 in ratios                                                  # w / wc and h / hc are not all 1
    # the tie cases' equal maxima lie a segment apart (56 rows at 224 x 56) and, at 224 x 224, more than a wave (64 columns) apart, in most channels (a
    # maximum in the clamped border band repeats along the border only)
    for i in (27, 28):
        hc, wc = cases[i][:2]
        tall = wide = 0
        for k in range(17):
            r = k64.resize(heat[i][:, :, k], hc, wc)
            ys, xs = np.nonzero(r == r.max())
            tall += int(ys.max() - ys.min() >= 56)
            wide += int(xs.max() - xs.min() > 64)
        print("tie case %d x %d: maxima a segment apart in %d channels, a wave apart in %d" % (hc, wc, tall, wide))
        assert tall >= 8 and (wide >= 8 or wc == 56), (hc, wc, tall, wide)


def altered_resize(m, hc, wc, a=-0.75, wrap=False, vertical_first=False, perturb=0.0, half=0.5):
    """The restatement with its decisions as parameters; the defaults give keypoint_ref.resize_bicubic's bits."""
    m = np.ascontiguousarray(m, F)
    S = m.shape[0]
    a = F(a)

    def taps(n_out):
        d = np.arange(n_out, dtype=F)
        f = (d + F(0.5)) * (F(S) / F(n_out)) - F(half)
        sf = np.floor(f)
        t = f - sf
        u, x = F(1.0) - t, t + F(1.0)
        w0 = ((a * x - F(5) * a) * x + F(8) * a) * x - F(4) * a
        w1 = (((a + F(2)) * t - (a + F(3))) * t) * t + F(1.0)
        w2 = (((a + F(2)) * u - (a + F(3))) * u) * u + F(1.0)
        w3 = ((F(1.0) - w0) - w1) - w2
        idx = sf.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
        return (idx % S if wrap else np.clip(idx, 0, S - 1)), np.stack([w0, w1, w2, w3], 1)

    xi, wx = taps(wc)
    yi, wy = taps(hc)
    if perturb:
        wy = wy.copy()
        wy[:, 1] = wy[:, 1] * F(1.0 + perturb)
    if vertical_first:
        cols = ((wy[:, 0, None] * m[yi[:, 0]] + wy[:, 1, None] * m[yi[:, 1]]) + wy[:, 2, None] * m[yi[:, 2]]) + wy[:, 3, None] * m[yi[:, 3]]   # [hc, S]
        return ((wx[:, 0] * cols[:, xi[:, 0]] + wx[:, 1] * cols[:, xi[:, 1]]) + wx[:, 2] * cols[:, xi[:, 2]]) + wx[:, 3] * cols[:, xi[:, 3]]
    rows = ((wx[:, 0] * m[:, xi[:, 0]] + wx[:, 1] * m[:, xi[:, 1]]) + wx[:, 2] * m[:, xi[:, 2]]) + wx[:, 3] * m[:, xi[:, 3]]
    return ((wy[:, 0, None] * rows[yi[:, 0]] + wy[:, 1, None] * rows[yi[:, 1]]) + wy[:, 2, None] * rows[yi[:, 2]]) + wy[:, 3, None] * rows[yi[:, 3]]


ALTERED = {"A = -0.5": dict(a=-0.5), "wrapped taps": dict(wrap=True), "vertical first, one weight off by 2^-12": dict(vertical_first=True, perturb=2.0 ** -12),
           "no - 0.5": dict(half=0.0)}
BOUND_CHANNELS = (0, 3, 8, 10, 11, 16)   # two corners, a segment edge, the second stride, two smooth-peak maps


def test_bound_holds_for_the_restatement_and_breaks_for_four_altered_ones():
    """Every map of the thread-layout sweep (133 sizes x 17 channels): |restatement - fp64| <= e elementwise, and the decode's answer passes
    keypoint_fp64.against_bound.  Measured: largest err / e 0.32.  Then six channels of every size through each altered restatement: its largest err / e
    must exceed 1 -- at every one of the 133 sizes for the wrong A, the wrong order + weight and the missing - 0.5; wrapped taps differ only where a tap
    leaves the map, so on channel 0, whose peak sits in the corner, they must break the bound at the 118 sizes with a side of 57 or more (at hc <= 5 and
    wc <= 3 no tap leaves the map in either axis, and wrapping is clamping)."""
    heat, boxes, count, kpt, ks, pos = ke.sweep_batch()
    worst = worst_score = worst_gap = 0.0
    broken = {name: 0 for name in ALTERED}
    worst_alt = {name: 0.0 for name in ALTERED}
    plain_order, wrapped_whole = 0.0, set()
    for n, hc in enumerate(ke.SWEEP_HC):
        for c, wc in enumerate(ke.SWEEP_WC):
            maps = heat[n * ke.SWEEP_CAP + c]
            size_broken = {name: False for name in ALTERED}
            for k in range(17):
                r64, e, _ = k64.resize_with_bound(maps[:, :, k], hc, wc)
                r32 = kr.resize_bicubic(maps[:, :, k], hc, wc)
                assert np.array_equal(r32, altered_resize(maps[:, :, k], hc, wc))
                worst = max(worst, float((np.abs(r32.astype(np.float64) - r64) / e).max()))
                a, b = k64.against_bound(maps[:, :, k], hc, wc, ks[n, c, k], int(pos[(n, c)][k]))
                worst_score, worst_gap = max(worst_score, a), max(worst_gap, b)
                if k in BOUND_CHANNELS:
                    plain_order = max(plain_order, float((np.abs(altered_resize(maps[:, :, k], hc, wc, vertical_first=True).astype(np.float64) - r64) / e).max()))
                    for name, kw in ALTERED.items():
                        if name == "wrapped taps" and k != 0:
                            continue
                        ratio = float((np.abs(altered_resize(maps[:, :, k], hc, wc, **kw).astype(np.float64) - r64) / e).max())
                        worst_alt[name] = max(worst_alt[name], ratio)
                        size_broken[name] |= ratio > 1.0
            for name in ALTERED:
                broken[name] += size_broken[name]
            if not size_broken["wrapped taps"]:
                wrapped_whole.add((hc, wc))
    print("restatement vs fp64 on the sweep: largest err / e %.4f; score %.4f of its bound, arg-max gap %.4f of its bound; vertical pass first alone %.4f"
          % (worst, worst_score, worst_gap, plain_order))
    print("altered restatements, sizes (of 133) that break the bound / largest err / e:", {k: (broken[k], "%.3g" % worst_alt[k]) for k in ALTERED})
    assert worst <= 1.0 and worst_score <= 1.0 and worst_gap <= 1.0
    assert plain_order <= 1.0                      # the order of the passes alone is inside the bound: it is the perturbed weight that breaks it
    assert broken == {name: 118 if name == "wrapped taps" else 133 for name in ALTERED}, broken
    assert wrapped_whole == {(hc, wc) for hc in ke.SWEEP_HC[:5] for wc in ke.SWEEP_WC[:3]}


def test_sweep_hits_every_place_and_every_layout():
    heat, boxes, count, kpt, ks, pos = ke.sweep_batch()
    assert boxes.shape == (7, 20, 4) and count.tolist() == [19] * 7 and np.isnan(heat[19]).all() and not kpt[:, 19].any()
    hit = ke.places_hit()
    print({k: len(v) for k, v in hit.items()})
    for name in ke.PLACES:
        # on a detection with several segments (wc 63 .. 128: nseg 4, 3, 2), one with a single full-width segment, and one whose columns are strided
        assert any(hc >= 57 and 63 <= wc <= 128 for hc, wc in hit[name]), name
        assert any(hc >= 57 and 129 <= wc <= 256 for hc, wc in hit[name]), name
        assert any(hc >= 57 and wc > 256 for hc, wc in hit[name]), name
    assert {wc for hc, wc in hit["second-stride"] if wc > 256} == {257, 300, 511, 512, 513, 1023}
    # the segment rows really are segment edges, and hc < nseg leaves segments empty
    assert ke.layout(63, 200) == (63, 4, 50) and ke.middle_segment(63, 200) == (100, 149) and ke.layout(86, 57) == (86, 2, 29) and ke.middle_segment(86, 57) == (29, 56)
    assert ke.layout(1, 5) == (1, 256, 1) and ke.middle_segment(1, 5) == (4, 4) and ke.layout(3, 200) == (3, 85, 3) and ke.middle_segment(3, 200) == (126, 128)
    for hc in (57, 200):
        for wc in (63, 64, 65, 85, 86, 127, 128):
            assert (hc, wc) in hit["segment-first-row"] and (hc, wc) in hit["segment-last-row"], (hc, wc)
    assert np.isfinite(kpt).all() and np.isfinite(ks).all()


def test_non_finite_expectations_of_the_restatement():
    """np.argmax's contract on the restatement: a NaN of the resized map is maximal and the first one wins."""
    heat, boxes, count, kpt, ks, pos = ke.nan_batch()
    assert np.isfinite(kpt).all() and (kpt[..., 2] == 1).all()
    for n, (hc, wc) in enumerate(ke.NAN_SIZES):
        assert kr.box_sizes(boxes[n, 0])[2:] == (wc, hc)
        by = {kind: c for c, kind in enumerate(ke.NAN_KINDS)}
        for kind in ("nan-mid", "nan-last-row"):
            c = by[kind]
            assert np.isnan(ks[n, c]).all()
            for k in (0, 16):
                with np.errstate(invalid="ignore"):
                    r = kr.resize_bicubic(heat[n * 6 + c][:, :, k], hc, wc).reshape(-1)
                first = int(np.nonzero(np.isnan(r))[0][0])
                assert pos[n, c, k] == first > 0 and not np.isnan(r).all()
        assert (pos[n, by["nan-last-row"]] // wc > hc * 0.9).all()                          # met by the last segment only
        assert (pos[n, by["all-nan"]] == 0).all() and np.isnan(ks[n, by["all-nan"]]).all()
        b = boxes[n, by["all-nan"]]
        assert (kpt[n, by["all-nan"], :, 0] > b[0]).all() and (kpt[n, by["all-nan"], :, 0] < b[0] + 1).all() and (kpt[n, by["all-nan"], :, 1] < b[1] + 1).all()
        # an all -inf map: the cubic weights have both signs (and zeros), so every resized value is inf - inf or 0 * inf: position 0, score NaN
        assert (pos[n, by["all-neg-inf"]] == 0).all() and np.isnan(ks[n, by["all-neg-inf"]]).all()
        c = by["inf-one"]
        assert (np.isnan(ks[n, c]) | (ks[n, c] == np.inf)).all() and (pos[n, c] > 0).all()
        c = by["nan-one-channel"]
        assert np.isnan(ks[n, c, ke.NAN_CHANNEL]) and np.isfinite(np.delete(ks[n, c], ke.NAN_CHANNEL)).all()
        clean = kr.decode_one(ke.sweep_maps(50 + c, 112, 112), boxes[n, c])
        keep = np.arange(17) != ke.NAN_CHANNEL
        assert np.array_equal(kpt[n, c][keep], clean[0][keep]) and np.array_equal(ks[n, c][keep], clean[1][keep])
    assert np.isnan(ks[1, by["inf-one"]]).any() and (ks[:, by["inf-one"]] == np.inf).any()  # both outcomes of an inf pixel occur
    assert ke.same_floats(np.array([np.nan, 1.0, -0.0], F), np.array([-np.nan, 1.0, -0.0], F)) and not ke.same_floats(np.array([0.0], F), np.array([-0.0], F))


def test_limit_cases():
    for s in (1, 2, 3, 64):
        for k in (1, 32):
            heat, boxes, count, kpt, ks = ke.limit_batch(s, k)
            assert heat.shape == (5, s, s, k) and count.tolist() == [4] and kpt.shape == (1, 5, k, 3) and np.isfinite(kpt[0, :4]).all() and not kpt[0, 4].any()
            assert [kr.box_sizes(b)[2:] for b in boxes[0, :4]] == [(wc, hc) for hc, wc in ke.LIMIT_SIDES]
    heat, boxes, count, kpt, ks = ke.grid_batch()
    assert heat.shape == (65535, 2, 2, 1) and boxes.shape == (255, 257, 4) and heat.nbytes == 1048560
    assert count.min() == 0 and count.max() == 257 and ((count > 0) & (count < 257)).any()
    for n, c in ((1, 0), (7, 0), (254, 100)):
        assert c < count[n]
        a, b, _ = kr.decode_one(heat[n * 257 + c], boxes[n, c])
        assert np.array_equal(a, kpt[n, c]) and np.array_equal(b, ks[n, c])
    assert not kpt[0].any() and not kpt[1, count[1]:].any() and kpt[7, :count[7], 0, 2].all()
    heat, boxes, count, kpt, ks = ke.long_batch()
    assert [kr.box_sizes(b)[2:] for b in boxes[0]] == [(1, 16384), (16384, 1), (16384, 2)]
    assert float(kr.box_sizes(boxes[0, 2])[0]) == 20000.0 and kr.MAX_SIDE == 16384
    assert kpt[0, 2, :, 0].max() <= 20000.5 and len(set(kpt[0, 2, :, 0].tolist())) > 8      # the cut width still spans the box: cw = 20000 / 16384
