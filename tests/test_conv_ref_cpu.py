"""The CPU oracle held to tests/conv_ref.py, without a GPU: the fp64 reference, the order-free exact inputs, the rounding bound and the edge generators
are trusted by the GPU files (tests/test_conv_exact_gpu.py, tests/test_conv_edges_gpu.py) only because the oracle -- an independent restatement, the
k-ordered fmaf chain of oracle/ora_ops.c -- meets them here at the very same shapes.  torch's fp64 conv2d is the second opinion on the reference itself."""
import numpy as np
import pytest

import conv_cases as cc
import conv_ref as ref
from oracle import ora


def _ora(ops, case, act, use_res, **kw):
    return ora.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"] if use_res else None, act, **kw)


@pytest.mark.parametrize("case", cc.EXACT_CASES + [cc.bm_edge_case(m) for m in (63, 144, 257)])
def test_oracle_is_exact_on_the_order_free_inputs(case):
    ops, vs = ref.exact_case(case)
    for (act, use_res), v in vs.items():
        assert ref.same_bits(_ora(ops, case, act, use_res), ref.expected_f32(v)), (act, use_res)
    for (act, use_res), v in vs.items():
        assert ref.same_bits(_ora(ops, case, act, use_res, ksplit=4), ref.expected_f32(v)), ("ksplit", act, use_res)


def test_big_shift_case_rounds_at_the_fp16_store():
    ops, vs = ref.exact_case(cc.BIG_SHIFT_CASE, big_shift=True)
    for (act, use_res), v in vs.items():
        assert ref.same_bits(_ora(ops, cc.BIG_SHIFT_CASE, act, use_res), ref.expected_f32(v))
        e16 = ref.expected_f16(v)
        assert np.isfinite(e16).all() and (e16.astype(np.float64) != v).mean() > 0.05   # half-integers above 2048: ties and plain roundings


@pytest.mark.parametrize("case", cc.F32_CASES + cc.F32_HYBRID_CASES[1:])
def test_oracle_is_exact_on_the_order_free_inputs_fp32_cases(case):
    ops, vs = ref.exact_case(case)
    for (act, use_res), v in vs.items():
        assert ref.same_bits(_ora(ops, case, act, use_res), ref.expected_f32(v)), (act, use_res)


@pytest.mark.parametrize("case", cc.EDGE_CASES)
def test_oracle_inside_the_bound_on_real_inputs(case):
    ops = ref.real_operands(case)
    worst = 0.0
    for act, use_res in ref.VARIANTS:
        res = ops["residual"] if use_res else None
        v = ref.conv2d_fp64(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act)
        e = ref.bound(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res)
        assert e.min() > 0
        for ks in (1, 4):
            got = _ora(ops, case, act, use_res, ksplit=ks).astype(np.float64)
            worst = max(worst, float((np.abs(got - v) / e).max()))
            assert np.all(np.abs(got - v) <= e), (ks, act, float((np.abs(got - v) / e).max()))
            assert np.all(ref.f16_inside(ref.h(got), v, e))
    print("case %s: oracle max |err| / e = %.4f" % (case, worst))


def test_bracket_helpers():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 65504.0, 65519.0, 65520.0, -65520.0, 1e-9, -1e-9, 0.0, 2049.0])
    lo, hi = ref.f16_at_or_below(v), ref.f16_at_or_above(v)
    assert lo.dtype == np.float16 and np.all(lo.astype(np.float64) <= v) and np.all(hi.astype(np.float64) >= v)
    assert np.array_equal(lo.astype(np.float64), [1.0, 1.0, 65504.0, 65504.0, 65504.0, -np.inf, 0.0, -2.0 ** -24, 0.0, 2048.0])
    assert np.array_equal(hi.astype(np.float64), [1.0, 1.0 + 2.0 ** -10, 65504.0, np.inf, np.inf, -65504.0, 2.0 ** -24, 0.0, 0.0, 2050.0])
    assert ref.f16_inside(np.array([1.0], np.float16), np.array([1.0003]), np.array([1e-9]))[0]          # the fp16 neighbours of v are always admitted
    assert not ref.f16_inside(np.array([1.002], np.float16), np.array([1.0003]), np.array([1e-9]))[0]    # and the one after is not


# ---------------------------------------------------------------- edges
NF_CASES = [(2, 19, 23, 64, 48, 3, 1, 1), (2, 35, 33, 128, 128, 3, 2, 1), (1, 35, 35, 64, 64, 1, 1, 0), (3, 14, 14, 128, 96, 3, 1, 1)]


@pytest.mark.parametrize("kind", ref.NONFINITE_KINDS)
@pytest.mark.parametrize("case", NF_CASES)
def test_oracle_on_non_finite_inputs(case, kind):
    ops, xd, m = ref.nonfinite_operands(case, kind)
    assert m.mean() <= 0.5
    for act, use_res in ref.VARIANTS:
        res = ops["residual"] if use_res else None
        clean = ora.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act)
        dirty = ora.conv2d(xd, ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act)
        with np.errstate(invalid="ignore", over="ignore"):
            v = ref.conv2d_fp64(xd, ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act).astype(np.float32)
        assert ref.same_bits(dirty[~m], clean[~m])                       # locality
        assert ref.same_values(dirty, v)                                 # inf with its sign, NaN where the reference has NaN, exact elsewhere
        assert act == 1 or not np.isfinite(v[m]).any()                   # every reachable output meets a non-finite product
        if act == 1:
            assert not np.isnan(dirty).any()                             # NaN through ReLU is 0 (`y > 0 ? y : 0`)
        else:
            assert np.isnan(dirty[m]).any() == (kind in ("nan", "mixed") or bool((ops["w"] == 0).any()))


@pytest.mark.parametrize("where", ["x", "w", "both"])
def test_oracle_keeps_fp16_subnormal_operands(where):
    case = (2, 9, 10, 64, 40, 3, 1, 1)
    ops, f = ref.subnormal_operands(case, where)
    got = ora.conv2d(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0)
    v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0)
    assert np.abs(v).max() > 0 and ref.same_bits(got, ref.expected_f32(v))
    assert np.array_equal(v / f, np.round(v / f))


@pytest.mark.parametrize("where", ["x", "product"])
def test_oracle_keeps_fp32_subnormals(where):
    case = (2, 9, 10, 64, 40, 3, 1, 1)
    ops, f = ref.f32_subnormal_operands(case, where)
    got = ora.conv2d(ops["x"], ops["w"], 1, 1, None, None, None, 0)
    v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 1)
    assert 0 < np.abs(v).max() < ref.F32_MIN_NORMAL and ref.same_bits(got, ref.expected_f32(v))


@pytest.mark.parametrize("Cout", [8, 9, 24])
def test_oracle_at_the_top_of_fp16(Cout):
    ops, t = ref.overflow_operands(Cout)
    for act in (0, 1):
        got = ora.conv2d(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act)
        v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act)
        assert np.array_equal(v[0, 0, 0], np.where((act == 1) & (t < 0), 0.0, t))
        assert ref.same_bits(got, ref.expected_f32(v))
    e16 = ref.expected_f16(ref.conv2d_fp64(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"]))[0, 0, 0, :6].astype(np.float64)
    assert np.array_equal(e16, [65504.0, 65504.0, 65504.0, np.inf, np.inf, np.inf])


def test_oracle_negative_zero():
    ops = ref.negative_zero_operands(16)
    for act, want in ((0, 0x80000000), (1, 0)):
        got = ora.conv2d(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act)
        v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act)
        assert np.all(ref.bits(v.astype(np.float32)) == want) and ref.same_bits(got, v.astype(np.float32))


def test_zero_input_with_shift_pads_the_bottleneck_halo_with_zero():
    """All-zero x and a positive shift in bn1: t1 = relu(shift) > 0 at every pixel INSIDE the image and 0 in the 3x3's padding, so conv2's border
    outputs differ from its interior ones; a t1 halo filled with relu(shift) would make them equal."""
    Cin, Cmid = 256, 64
    x, w1, sb1, w2, sb2, w3, sb3 = ref.bottleneck_operands((Cin, Cmid), (1, 6, 7))
    x = np.zeros_like(x); sb1 = (sb1[0], np.abs(sb1[1]) + 1.0); w2 = np.abs(w2)
    out, t1, t2 = ref.bottleneck_fp64(x, w1, sb1, w2, sb2, w3, sb3, return_inner=True)
    assert (t1 > 0).all() and np.array_equal(t1[0, 0, 0], sb1[1])
    pre = ref.conv_acc_fp64(t1, w2, 1, 1)
    assert np.all(pre[0, 0, 0] < pre[0, 2, 3]) and np.array_equal(pre[0, 2, 3], pre[0, 3, 3])
    t1o = ora.conv2d(x, w1, 1, 0, sb1[0], sb1[1], None, 1)
    t2o = ora.conv2d(t1o, w2, 1, 1, sb2[0], sb2[1], None, 1)
    oo = ora.conv2d(t2o, w3, 1, 0, sb3[0], sb3[1], x, 1)
    assert ref.same_bits(oo, ref.expected_f32(out))


# ---------------------------------------------------------------- fused references
@pytest.mark.parametrize("ch", cc.BOTTLENECK_CH)
@pytest.mark.parametrize("projection", [False, True])
def test_bottleneck_operands_have_one_right_answer(ch, projection):
    if projection:
        ch = (64, 64)
    for shape in cc.BOTTLENECK_SHAPES[:4]:
        ops = ref.bottleneck_operands(ch, shape, projection)
        out, t1, t2 = ref.bottleneck_fp64(*ops, return_inner=True)
        x, w1, sb1, w2, sb2 = ops[:5]
        # t1 / t2 are fp16 numbers before they are rounded, below 2048 (so the rounding of the contract changes nothing)
        assert np.array_equal(t1, ref.conv2d_fp64(x, w1, 1, 0, sb1[0], sb1[1], None, 1)) and t1.max() < 2048
        assert np.array_equal(t2, ref.conv2d_fp64(t1, w2, 1, 1, sb2[0], sb2[1], None, 1)) and t2.max() < 2048
        assert len(np.unique(t1)) >= 20 and len(np.unique(t2)) >= 50 and len(np.unique(out)) >= 50 and out.max() < ref.F16_MAX
        ref.expected_f16(out)
        t1o = ora.conv2d(x, w1, 1, 0, sb1[0], sb1[1], None, 1)
        t2o = ora.conv2d(t1o, w2, 1, 1, sb2[0], sb2[1], None, 1)
        sc = x if not projection else ora.conv2d(x, ops[7], 1, 0, ops[8][0], ops[8][1], None, 0)
        assert ref.same_bits(ora.conv2d(t2o, ops[5], 1, 0, ops[6][0], ops[6][1], sc, 1), ref.expected_f32(out))


@pytest.mark.parametrize("shape", cc.STEM_SHAPES[:5])
def test_stem_reference_against_the_oracle(shape):
    x, w, scale, shift = ref.stem_operands(shape)
    v = ref.stem_fp64(x, w, scale, shift)
    x4 = np.concatenate([x, np.zeros(x.shape[:3] + (1,), np.float32)], -1)
    assert ref.same_bits(ora.conv2d(x4, w, 2, 3, scale, shift, None, 1), ref.expected_f32(v))
    e16 = ref.expected_f16(v)
    assert np.isfinite(e16).all() and len(np.unique(e16)) >= 50 and (e16.astype(np.float64) != v).mean() > 0.05
    pooled = ref.maxpool3x3s2_f16(e16)
    assert ref.same_bits(pooled, ora.maxpool(e16.astype(np.float32), 3, 2, 1).astype(np.float16))


@pytest.mark.parametrize("case", cc.MERGE_CASES[:5] + cc.MERGE_CASES[8:9])
def test_merge_reference_against_the_oracle(case):
    x, w, scale, shift, coarse = ref.merge_operands(case)
    v = ref.merge_fp64(x, w, scale, shift, coarse)
    lat = ora.conv2d(x, w, 1, 0, scale, shift, None, 0).astype(np.float16).astype(np.float32)
    N, H, W, Cin, Hc, Wc = case
    if (Hc, Wc) == ((H + 1) // 2, (W + 1) // 2):
        assert ref.same_bits(ora.upsample_nearest2x_add(coarse, lat), ref.expected_f32(v))
    assert np.abs(v).max() < ref.F16_MAX and len(np.unique(v)) >= 50


@pytest.mark.parametrize("case", [(1, 20, 31, 256, 15), (1, 9, 40, 64, 3)])
def test_head_reference_against_the_oracle(case):
    x, w, scale, shift, w2, scale2, shift2 = ref.head_operands(case)
    v, t = ref.head_fp64(x, w, scale, shift, w2, scale2, shift2)
    to = ora.conv2d(x, w, 1, 1, scale, shift, None, 1).astype(np.float16).astype(np.float32)
    assert ref.same_bits(to, t.astype(np.float32))
    assert ref.same_bits(ora.conv2d(to, w2, 1, 0, scale2, shift2, None, 0), ref.expected_f32(v))


# ---------------------------------------------------------------- strided output form
STRIDED = [  # case, img_stride, pix_stride, offset, out elements (the oracle addresses by image: its out_div is always Ho * Wo)
    # one of the four taps of the mask head's 2x2 deconvolution (out_div = 14 of a 14 x 14 map), restated as 3 * 14 one-row images so that Ho * Wo = 14
    ((3 * 14, 1, 14, 64, 256, 1, 1, 0), 2 * 28 * 256, 2 * 256, 28 * 256 + 256, 3 * 28 * 28 * 256),
    ((2, 9, 10, 64, 15, 3, 1, 1), 500 * 15, 15, 37 * 15, 2 * 500 * 15),                          # a head's slice of the concatenated [N][P][C] buffer
    ((2, 9, 10, 64, 8, 3, 1, 1), 2000, 20, 3, 4100),                                             # strides that break 16-byte alignment
]


@pytest.mark.parametrize("spec", STRIDED)
def test_oracle_strided_output_is_the_reference_scatter(spec):
    case, istr, pstr, off, n = spec
    div = cc.m_of(case) // case[0]
    ops = ref.exact_operands(case, key="strided")
    v = ref.conv2d_fp64(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, 1)
    want, mask = ref.scatter(ref.expected_f32(v).reshape(-1, case[4]), (n,), np.float32, div, istr, pstr, off)
    out = np.frombuffer(b"\xff" * (4 * n), np.float32).copy()
    ora.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, 1, out=out[off:], out_img_stride=istr, out_pix_stride=pstr)
    assert mask.sum() == v.size
    assert ref.same_bits(out, want) and np.all(ref.bits(out)[~mask] == 0xFFFFFFFF)


def test_scatter_with_an_out_div_that_does_not_divide_m():
    """ref.scatter itself on the form the oracle cannot express (out_div = 7 over M = 90 pixels): every element lands once, at the stated index."""
    v = np.arange(90 * 8, dtype=np.float64).reshape(90, 8)
    want, mask = ref.scatter(v, (1300,), np.float32, 7, 100, 12, 0)
    assert mask.sum() == v.size and np.all(ref.bits(want)[~mask] == 0xFFFFFFFF)
    for m in (0, 6, 7, 89):
        assert np.array_equal(want[(m // 7) * 100 + (m % 7) * 12:][:8], v[m])


def test_deconv2x2_is_four_strided_1x1_convolutions():
    rng = cc.rng_for("deconv")
    R_, C = 3, 64
    x = rng.integers(-2, 4, (R_, 14, 14, C)).astype(np.float32)
    w = rng.integers(-2, 3, (C, 32, 2, 2)).astype(np.float32)   # [Cin][Cout][2][2]
    b = rng.integers(-8, 9, 32).astype(np.float32)
    want = ora.deconv2x2(x, w, b, 1)
    out = np.frombuffer(b"\xff" * (4 * R_ * 28 * 28 * 32), np.float32).copy().reshape(R_, 28, 28, 32)
    for a in range(2):
        for bb in range(2):
            v = ref.conv2d_fp64(x, w[:, :, a, bb].T.reshape(32, 1, 1, C), 1, 0, None, b, None, 1)
            part, mask = ref.scatter(v.reshape(-1, 32), out.shape, np.float32, 14, 2 * 28 * 32, 2 * 32, (a * 28 + bb) * 32)
            out[mask] = part[mask]
    assert ref.same_bits(out, want)


def test_reference_against_torch_fp64():
    torch = pytest.importorskip("torch")
    for case in [(2, 19, 23, 64, 48, 3, 1, 1), (2, 35, 33, 128, 128, 3, 2, 1), (1, 7, 7, 256, 64, 7, 1, 0)]:
        ops = ref.real_operands(case)
        v = ref.conv2d_fp64(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"], 1)
        t = torch.nn.functional.conv2d(torch.from_numpy(ops["x"].astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(ops["w"].astype(np.float64)).permute(0, 3, 1, 2),
                                       stride=case[6], padding=case[7]).permute(0, 2, 3, 1).numpy()
        t = np.maximum(t * ops["scale"].astype(np.float64) + ops["shift"].astype(np.float64) + ops["residual"].astype(np.float64), 0)
        a = ref.abs_sum(ops["x"], ops["w"], case[6], case[7])
        assert np.all(np.abs(t - v) <= 2.0 ** -50 * cc.k_of(case) * (a * 1.5 + 10))   # two fp64 summations of the same K products
        ops, vs = ref.exact_case(case) if case in cc.EXACT_CASES else (None, None)
        if ops is not None:
            t = torch.nn.functional.conv2d(torch.from_numpy(ops["x"].astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(ops["w"].astype(np.float64)).permute(0, 3, 1, 2),
                                           stride=case[6], padding=case[7]).permute(0, 2, 3, 1).numpy()
            assert np.array_equal(t * ops["scale"].astype(np.float64) + ops["shift"].astype(np.float64), vs[(0, False)])


# ---------------------------------------------------------------- the skip rule, as a table
def test_skip_rule_leaves_every_tile_enough_cases():
    pairs = [(t, c) for t in cc.F16_TILES for c in cc.EXACT_CASES]
    refused = [(t, c) for t, c in pairs if cc.f16_refused(t, c)]
    assert len(refused) * 3 <= len(pairs), (len(refused), len(pairs))
    for t in cc.F16_TILES:
        assert sum(cc.f16_refused(t, c) is None for c in cc.EXACT_CASES) >= 3, t
        assert sum(cc.f16_refused(t, c) is None and cc.k_of(c) >= cc.DEEP_K for c in cc.EDGE_CASES) >= 1, t
        assert all(cc.f16_refused(t, cc.bm_edge_case(m)) is None for m in cc.BM_EDGES), t
    # the rule itself, on hand-made pairs
    assert cc.f16_refused(30, (1, 9, 9, 64, 8, 1, 1, 0)) and cc.f16_refused(40, (1, 9, 9, 64, 8, 3, 2, 1)) and cc.f16_refused(4, (1, 9, 9, 32, 8, 3, 1, 1))
    assert cc.f16_refused(27, (1, 9, 8, 64, 8, 3, 1, 1)) and not cc.f16_refused(27, (1, 9, 9, 64, 8, 3, 1, 1))       # 255 / 8 + 2 = 33
    assert cc.f16_refused(30, (1, 9, 6, 64, 8, 3, 1, 1)) and not cc.f16_refused(30, (1, 9, 7, 64, 8, 3, 1, 1))       # 191 / 6 + 2 = 33
    assert cc.f16_refused(41, (1, 9, 4, 64, 8, 3, 1, 1)) and not cc.f16_refused(41, (1, 9, 5, 64, 8, 3, 1, 1))       # 143 / 4 + 2 = 37
    assert cc.f16_refused(cc.FEW + 37, (1, 9, 1, 64, 8, 3, 1, 1)) is None
    assert sorted(set(t & 255 for t in cc.F16_TILES) - {0}) == sorted(cc.F16_BM)
    # every BM has its M - 1 / M / M + 1
    assert all(bm + d in cc.BM_EDGES for bm in set(cc.F16_BM.values()) for d in (-1, 0, 1))
    # every persistent tile has a case whose cdiv(M, BM) x cdiv(Cout, BN) tiles are more than 8 and leave the split over the 8 XCDs a remainder
    for t in cc.F16_PERSIST + cc.F16_M16_PERSIST:
        totals = [-(-cc.m_of(c) // cc.F16_BM[t]) * -(-c[4] // cc.F16_PERSIST_BN[t]) for c in cc.EXACT_CASES]
        assert any(n > 8 and n % 8 for n in totals), (t, totals)
