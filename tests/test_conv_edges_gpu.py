"""The conv kernels on real-valued and edge inputs, against the fp64 reference, the derived rounding bound and the oracle's own error
(tests/conv_ref.py; the oracle is held to the same references in tests/test_conv_ref_cpu.py): deep K, non-finite activations and how far they
reach, subnormal operands, the top of the fp16 range at the store, signed zeros, the strided output mode with every untouched byte checked, and
launch-to-launch determinism."""
import numpy as np
import pytest

import conv_cases as cc
import conv_ref as ref
from oracle import ora

pytestmark = pytest.mark.gpu

FAMILY_TILES = sorted(set(cc.F16_FAMILY.values()))
_real = {}


def _real_case(case):
    """-> operands, {(act, res): (v, e, rms of the oracle's error)}: once per case."""
    if case not in _real:
        ops = ref.real_operands(case)
        d = {}
        for act, use_res in ref.VARIANTS:
            res = ops["residual"] if use_res else None
            v = ref.conv2d_fp64(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act)
            e = ref.bound(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res)
            o = ora.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act)
            assert np.all(np.abs(o - v) <= e)
            d[(act, use_res)] = (v, e, ref.rms(o - v), o)
        _real[case] = (ops, d)
    return _real[case]


@pytest.mark.parametrize("case", cc.EDGE_CASES)
@pytest.mark.parametrize("tile", cc.F16_TILES)
def test_f16_conv_inside_the_bound_and_the_oracles_rms(ffi, case, tile):
    """fp32 output: |got - v| <= e and rms(got - v) <= 2 x rms(oracle - v).  fp16 output: got between the fp16 neighbours of v -+ e, and >= 99 % equal
    to the rounded oracle (the check of tests/test_conv_f16_gpu.py, kept)."""
    if cc.f16_refused(tile, case):
        pytest.skip(cc.f16_refused(tile, case))
    ops, d = _real_case(case)
    for (act, use_res), (v, e, ora_rms, o) in d.items():
        res = ops["residual"] if use_res else None
        g32 = ffi.conv2d_f16(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act, tile, out_f32=True)
        g16 = ffi.conv2d_f16(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act, tile)
        ratio = float((np.abs(g32 - v) / e).max()); r = ref.rms(g32 - v) / ora_rms   # (measured: conv_ref.py's docstring)
        assert ratio <= 1.0, ratio
        assert r <= ref.RMS_MARGIN, r
        assert np.all(ref.f16_inside(g16, v, e))
        assert np.mean(g16 == o.astype(np.float16)) >= 0.99


@pytest.mark.parametrize("case", cc.EDGE_CASES)
@pytest.mark.parametrize("tile", cc.F32_TILES)
def test_f32_conv_inside_the_bound(ffi, case, tile):
    """The fp32 kernels, every tile (15: the fixed-tree split-K, another association): inside e of the fp64 value, and no worse than twice the oracle
    chain's RMS error, on fp16-valued operands."""
    ops, d = _real_case(case)
    for (act, use_res), (v, e, ora_rms, o) in d.items():
        got = ffi.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"] if use_res else None, act, tile)
        assert np.all(np.abs(got - v) <= e) and ref.rms(got - v) <= ref.RMS_MARGIN * ora_rms


@pytest.mark.parametrize("shape", [(2, 50, 70), (1, 37, 45), (1, 64, 33)])
@pytest.mark.parametrize("tile", [0, 8])
def test_stem_f16_inside_the_bound(ffi, shape, tile):
    """The fp16 stem is one convolution (K = 147), so e is defined for it: real-valued image and weights, fp16 output between the fp16 neighbours of v -+ e."""
    rng = cc.rng_for("stem-real", shape)
    x = ref.h(rng.uniform(-120.0, 130.0, shape + (3,))).astype(np.float32)
    w = np.zeros((64, 7, 7, 4), np.float32)
    w[..., :3] = ref.h(rng.standard_normal((64, 7, 7, 3)) * (2.0 / 147.0) ** 0.5)
    scale = rng.uniform(0.5, 1.5, 64).astype(np.float32); shift = (rng.standard_normal(64) * 0.1).astype(np.float32)
    v = ref.stem_fp64(x, w, scale, shift)
    e = ref.bound(x, w[..., :3], 2, 3, scale, shift)
    got, _ = ffi.stem_f16(x, w, scale, shift, tile)
    assert np.all(ref.f16_inside(got, v, e))
    x4 = np.concatenate([x, np.zeros(shape + (1,), np.float32)], -1)
    assert np.mean(got == ora.conv2d(x4, w, 2, 3, scale, shift, None, 1).astype(np.float16)) >= 0.99


# ---------------------------------------------------------------- non-finite activations: where they reach and what they become
NF_CASES = [(2, 19, 23, 64, 48, 3, 1, 1), (2, 35, 33, 128, 128, 3, 2, 1), (1, 35, 35, 64, 64, 1, 1, 0), (3, 14, 14, 128, 96, 3, 1, 1)]


def _nf_check(run, case, kind, to16):
    ops, xd, m = ref.nonfinite_operands(case, kind)
    assert m.mean() <= 0.5
    for act, use_res in ref.VARIANTS:
        res = ops["residual"] if use_res else None
        clean, dirty = run(ops["x"], ops, res, act), run(xd, ops, res, act)
        with np.errstate(invalid="ignore", over="ignore"):
            v = ref.conv2d_fp64(xd, ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act).astype(np.float32)
        want = ref.h(v) if to16 else v
        assert ref.same_bits(dirty[~m], clean[~m]), "a non-finite input changed an output whose window does not hold it"
        assert ref.same_values(dirty, want), "%d elements differ" % int((ref.bits(dirty) != ref.bits(want)).sum())
        if act == 1:
            assert not np.isnan(dirty).any()    # NaN through ReLU is 0: `y > 0 ? y : 0`, in kernel, oracle and reference alike


@pytest.mark.parametrize("kind", ref.NONFINITE_KINDS)
@pytest.mark.parametrize("case", NF_CASES)
@pytest.mark.parametrize("tile", FAMILY_TILES)
def test_f16_conv_non_finite_locality(ffi, case, kind, tile):
    if cc.f16_refused(tile, case):
        pytest.skip(cc.f16_refused(tile, case))
    for f32 in (False, True):
        _nf_check(lambda x, ops, res, act: ffi.conv2d_f16(x, ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act, tile, out_f32=f32), case, kind, not f32)


@pytest.mark.parametrize("kind", ref.NONFINITE_KINDS)
@pytest.mark.parametrize("case", NF_CASES)
@pytest.mark.parametrize("tile", [0, 4, 10, 15])
def test_f32_conv_non_finite_locality(ffi, case, kind, tile):
    _nf_check(lambda x, ops, res, act: ffi.conv2d(x, ops["w"], case[6], case[7], ops["scale"], ops["shift"], res, act, tile), case, kind, False)


@pytest.mark.parametrize("kind", ["+inf", "nan"])
@pytest.mark.parametrize("flags", [0, 1])
def test_bottleneck_non_finite_locality(ffi, kind, flags):
    """One non-finite activation in x reaches the 3 x 3 neighbourhood (through conv2) and nothing else.  Inside it the result is compared where the
    reference is a number; where fp64 says NaN through the chain the kernel must say NaN or, after the ReLUs, what `y > 0 ? y : 0` makes of it."""
    ch, shape = (256, 64), (2, 19, 37)
    ops = ref.bottleneck_operands(ch, shape)
    x = ops[0].copy(); site = (1, 9, 20, 63)
    x[site] = {"+inf": np.inf, "nan": np.nan}[kind]
    m = ref.reach((2, 19, 37, 64, 64, 3, 1, 1), [site[:3]])
    clean, dirty = ffi.bottleneck_f16(*ops, flags=flags), ffi.bottleneck_f16(x, *ops[1:], flags=flags)
    assert m.sum() == 9 and ref.same_bits(dirty[~m], clean[~m])
    with np.errstate(invalid="ignore", over="ignore"):
        want = ref.h(ref.bottleneck_fp64(x, *ops[1:]))
    assert ref.same_values(dirty, want), "%d elements differ" % int((ref.bits(dirty) != ref.bits(want)).sum())
    assert not np.array_equal(ref.bits(dirty[m]), ref.bits(clean[m]))


def _stem_sets(N, H, W, site):
    """(the outputs whose 7x7 window holds the pixel, the outputs whose 8 x 8 zero-extended window holds it) of the 7x7 / 2 / pad 3 stem."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n, y, x = site
    yo, xo = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    m7 = np.zeros((N, Ho, Wo), bool); m8 = np.zeros((N, Ho, Wo), bool)
    m7[n] = (y - (2 * yo - 3) >= 0) & (y - (2 * yo - 3) < 7) & (x - (2 * xo - 3) >= 0) & (x - (2 * xo - 3) < 7)
    m8[n] = (y - (2 * yo - 3) >= 0) & (y - (2 * yo - 3) < 8) & (x - (2 * xo - 3) >= 0) & (x - (2 * xo - 3) < 8)
    return m7, m8


@pytest.mark.parametrize("val", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("tile", [0, 8])
def test_stem_f16_requires_finite_input(ffi, val, tile):
    """THE CONTRACT (numerics): the fp16 stem requires a finite image.  Its K layout is 8 rows x 8 taps x 4 channels with zero weights at
    row 7 and tap 7, which cover REAL pixels: a non-finite pixel there is multiplied by zero, 0 * inf = NaN, and the NaN goes through the ReLU as 0.
    So a non-finite pixel spoils every output whose 8 x 8 window holds it, not only those whose 7x7 window does; the product feeds the stem from uint8
    images through a finite normalisation, so it never meets this.  Pinned here: outside the 8 x 8 set nothing changes; inside the 7x7 set the result
    is the reference's (NaN -> 0 through the ReLU); in the ring between them every output is 0 where the clean result was whatever it was."""
    shape = (2, 37, 45)
    x, w, scale, shift = ref.stem_operands(shape)
    site = (1, 18, 20); xd = x.copy(); xd[site + (1,)] = val   # even y and x: row 7 AND tap 7 of some windows hold the pixel
    m7, m8 = _stem_sets(*shape, site)
    clean, _ = ffi.stem_f16(x, w, scale, shift, tile); dirty, _ = ffi.stem_f16(xd, w, scale, shift, tile)
    assert ref.same_bits(dirty[~m8], clean[~m8])
    with np.errstate(invalid="ignore", over="ignore"):
        want = ref.h(ref.stem_fp64(xd, w, scale, shift))
    assert ref.same_values(dirty[m7], want[m7])
    ring = m8 & ~m7
    assert m8.sum() == 16 and m7.sum() == 9 and ring.sum() == 7   # 4 x 4 windows hold the pixel, 3 x 3 of them inside their 7x7
    assert np.all(ref.bits(dirty[ring]) == 0), "0 * non-finite = NaN, and NaN through the ReLU is +0"


@pytest.mark.parametrize("flags", [0, 3])
def test_stem_pool_f16_non_finite_reach(ffi, flags):
    """The fused stem + pool under the same contract: pooled outputs whose 3x3 window holds no conv output of the 8 x 8 set are untouched."""
    shape = (2, 37, 45)
    x, w, scale, shift = ref.stem_operands(shape)
    site = (1, 18, 20); xd = x.copy(); xd[site + (1,)] = np.inf
    m7, m8 = _stem_sets(*shape, site)
    clean, dirty = ffi.stem_pool_f16(x, w, scale, shift, flags), ffi.stem_pool_f16(xd, w, scale, shift, flags)
    pm = ref.maxpool3x3s2_f16(m8[..., None].astype(np.float16))[..., 0] > 0
    assert pm.mean() < 0.5 and ref.same_bits(dirty[~pm], clean[~pm])
    conv, _ = ffi.stem_f16(xd, w, scale, shift, 0)
    assert ref.same_bits(dirty, ref.maxpool3x3s2_f16(conv))


# ---------------------------------------------------------------- subnormal operands
SUB_CASE = (2, 9, 10, 64, 40, 3, 1, 1)


@pytest.mark.parametrize("where", ["x", "w", "both"])
@pytest.mark.parametrize("tile", FAMILY_TILES)
def test_f16_conv_keeps_subnormal_operands(ffi, where, tile):
    """fp16 subnormals (k * 2^-24) in x, in w, in both: the f16 MFMA of gfx950 takes them at their value; the fp32 result is the exact
    integer result times the power of two, bit for bit equal to the fp64 reference and to the oracle.  The fp16 output keeps subnormal RESULTS too."""
    ops, f = ref.subnormal_operands(SUB_CASE, where)
    v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0)
    got = ffi.conv2d_f16(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0, tile, out_f32=True)
    assert ref.same_bits(got, ref.expected_f32(v))
    assert ref.same_bits(got, ora.conv2d(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0))
    if where != "both":
        g16 = ffi.conv2d_f16(ops["x"], ops["w"], 1, 1, ops["scale"], ops["shift"], None, 0, tile)
        assert ref.same_bits(g16, ref.expected_f16(v)) and (np.abs(g16) < ref.F16_MIN_NORMAL).mean() > 0.5


@pytest.mark.parametrize("where", ["x", "product"])
@pytest.mark.parametrize("tile", [0, 4, 10])
def test_f32_conv_subnormals_against_the_oracle(ffi, where, tile):
    """fp32 subnormal operands, and normal operands whose products are subnormal: the oracle's fmaf chain keeps them; the claim of bit-exactness of
    the fp32 kernels (tests/test_conv_gpu.py) is held to it here."""
    ops, f = ref.f32_subnormal_operands(SUB_CASE, where)
    v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 1)
    want = ora.conv2d(ops["x"], ops["w"], 1, 1, None, None, None, 0)
    assert ref.same_bits(want, ref.expected_f32(v))
    got = ffi.conv2d(ops["x"], ops["w"], 1, 1, None, None, None, 0, tile)
    assert ref.same_bits(got, want)


# ---------------------------------------------------------------- the top of fp16, signed zeros
@pytest.mark.parametrize("Cout", [24, 9])   # the vector epilogue (Cout % 8 == 0) and the per-element one
@pytest.mark.parametrize("tile", [t for t in FAMILY_TILES if t & 255 not in cc.F16_STRIP + cc.F16_M16_STRIP])   # (a 1x1: no strip tile)
def test_f16_store_at_the_top_of_the_range(ffi, Cout, tile):
    """65504 stays, 65519 and the last fp32 below 65520 round down to it, the 65520 tie and everything above become inf (both signs)."""
    ops, t = ref.overflow_operands(Cout)
    for act in (0, 1):
        v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act)
        got = ffi.conv2d_f16(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act, tile)
        assert ref.same_bits(got, ref.expected_f16(v))
        assert np.array_equal(got[0, 0, 0, :6].astype(np.float64), [65504.0, 65504.0, 65504.0, np.inf, np.inf, np.inf])
        assert ref.same_bits(ffi.conv2d_f16(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, act, tile, out_f32=True), ref.expected_f32(v))


@pytest.mark.parametrize("Cout", [16, 9])
def test_negative_zero_results(ffi, Cout):
    """y = fmaf(+0, -1, -0) = -0.  With ReLU every kernel stores +0 (`y > 0 ? y : 0`), as reference and oracle do; with a residual of -0 every kernel
    stores -0 + -0 = -0.  Without residual and without ReLU the SIGN of a zero result is outside the contract (some epilogues add
    a +0 residual unconditionally, and -0 + +0 = +0, where oracle and reference keep -0): there the result only has to be a zero."""
    ops = ref.negative_zero_operands(Cout)
    run16 = lambda r, act, tile, f32: ffi.conv2d_f16(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], r, act, tile, out_f32=f32)
    run32 = lambda r, act: ffi.conv2d(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], r, act, 0)
    v = ref.conv2d_fp64(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], None, 0)
    assert np.signbit(v).all() and not v.any()
    r = np.full(v.shape, -0.0, np.float32)
    assert np.all(ref.bits(ora.conv2d(ops["x"], ops["w"], 1, 0, ops["scale"], ops["shift"], r, 0)) == 0x80000000)
    for tile in (4, 37, cc.FEW + 46):
        for f32 in (False, True):
            assert not run16(None, 0, tile, f32).any(), (tile, f32)                      # a zero, either sign
            assert np.all(ref.bits(run16(None, 1, tile, f32)) == 0), (tile, f32)         # ReLU: +0
            assert np.all(ref.bits(run16(r, 0, tile, f32)) == (0x80000000 if f32 else 0x8000)), (tile, f32)   # -0 residual: -0
    assert not run32(None, 0).any()
    assert np.all(ref.bits(run32(None, 1)) == 0)
    assert np.all(ref.bits(run32(r, 0)) == 0x80000000)


# ---------------------------------------------------------------- strided outputs
def _strided(ffi, case, tile, f32, div, istr, pstr, off, n, act=1, fp32_kernel=False):
    ops = ref.exact_operands(case, key="strided")
    v = ref.conv2d_fp64(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, act)
    dt = np.float32 if (f32 or fp32_kernel) else np.float16
    want, mask = ref.scatter(ref.expected_f32(v).reshape(-1, case[4]), (n,), dt, div, istr, pstr, off)
    kw = dict(out_shape=(n,), out_div=div, out_img_stride=istr, out_pix_stride=pstr, out_offset=off)
    if fp32_kernel:
        got = ffi.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, act, tile, **kw)
    else:
        got = ffi.conv2d_f16(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, act, tile, out_f32=f32, **kw)
    ones = np.iinfo(ref.bits(got).dtype).max
    assert np.all(ref.bits(got)[~mask] == ones), "%d bytes outside the addressed elements were written" % int((ref.bits(got)[~mask] != ones).sum())
    assert ref.same_bits(got, want), "%d addressed elements differ" % int((ref.bits(got) != ref.bits(want)).sum())


STRIDED_TILES = [4, 17, 37, cc.FEW + 39, cc.FEW + 46, 0]   # generic, generic with loader waves, persistent, m16 persistent, the cost model's choice


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("tile", STRIDED_TILES)   # (the taps are 1x1: no strip tile)
def test_f16_strided_mask_head_scatter(ffi, tile, f32):
    """The mask head's 2x2 deconvolution as four 1x1 convolutions with out_div = 14 into [R, 28, 28, 256]: each tap writes its quarter of the
    pixels and leaves the other three quarters untouched; the four together are ora.deconv2x2 and the fp64 reference."""
    R_, C, Co = 5, 256, 256
    rng = cc.rng_for("maskhead")
    x = rng.integers(-2, 4, (R_, 14, 14, C)).astype(np.float32)
    w = (rng.integers(1, 3, (C, Co, 2, 2)) * rng.choice([-1, 1], (C, Co, 2, 2))).astype(np.float32)
    b = rng.integers(-8, 9, Co).astype(np.float32)
    dt = np.float32 if f32 else np.float16
    full = np.zeros((R_, 28, 28, Co), dt); count = np.zeros(full.shape, np.int32)
    n = full.size
    for a in range(2):
        for bb in range(2):
            wk = np.ascontiguousarray(w[:, :, a, bb].T).reshape(Co, 1, 1, C)
            v = ref.conv2d_fp64(x, wk, 1, 0, None, b, None, 1)
            want, mask = ref.scatter(ref.expected_f32(v).reshape(-1, Co), (n,), dt, 14, 2 * 28 * Co, 2 * Co, (a * 28 + bb) * Co)
            got = ffi.conv2d_f16(x, wk, 1, 0, None, b, None, 1, tile, out_f32=f32, out_shape=(n,), out_div=14, out_img_stride=2 * 28 * Co,
                                 out_pix_stride=2 * Co, out_offset=(a * 28 + bb) * Co)
            ones = np.iinfo(ref.bits(got).dtype).max
            assert np.all(ref.bits(got)[~mask] == ones) and ref.same_bits(got, want)
            full.reshape(-1)[mask] = got[mask]; count.reshape(-1)[mask] += 1
    assert (count == 1).all()
    assert ref.same_bits(full, ora.deconv2x2(x, w, b, 1).astype(dt))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("tile", STRIDED_TILES + [30, 40])
@pytest.mark.parametrize("Cout", [3, 12, 15, 324])
def test_f16_strided_head_concatenation(ffi, Cout, tile, f32):
    """A level's slice of the concatenated [N][sum P][C] prediction buffer (yolact.cpp: fp32 heads, Cout % 8 != 0 on the per-element epilogue)."""
    case = (2, 9, 10, 64, Cout, 3, 1, 1)
    _strided(ffi, case, tile, f32, 90, 500 * Cout, Cout, 37 * Cout, 2 * 500 * Cout, act=0)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("tile", STRIDED_TILES + [30, 40])
def test_f16_strided_unaligned_and_ragged_div(ffi, tile, f32):
    """Cout % 8 == 0 with a pixel stride / offset that breaks the 16-byte alignment (the launcher must leave the vector epilogue), with aligned strides
    (it stays on it), and an out_div that does not divide M."""
    _strided(ffi, (2, 9, 10, 64, 8, 3, 1, 1), tile, f32, 90, 2000, 20, 3, 4100)
    _strided(ffi, (2, 9, 10, 64, 16, 3, 1, 1), tile, f32, 90, 4000, 40, 8, 8200)
    _strided(ffi, (2, 9, 10, 64, 16, 3, 1, 1), tile, f32, 90, 3600, 40, 8, 7300)   # image stride = out_div x pixel stride: the walked-offset form of the epilogue
    _strided(ffi, (1, 9, 10, 64, 8, 3, 1, 1), tile, f32, 7, 120, 16, 0, 1600)
    _strided(ffi, (1, 9, 10, 64, 7, 3, 1, 1), tile, f32, 7, 100, 12, 5, 1400)


@pytest.mark.parametrize("tile", [0, 4, 10, 15])
def test_f32_strided_outputs(ffi, tile):
    for Cout in (3, 15, 324):
        _strided(ffi, (2, 9, 10, 64, Cout, 3, 1, 1), tile, True, 90, 500 * Cout, Cout, 37 * Cout, 2 * 500 * Cout, act=0, fp32_kernel=True)
    _strided(ffi, (2, 9, 10, 64, 8, 3, 1, 1), tile, True, 90, 2000, 20, 3, 4100, fp32_kernel=True)
    _strided(ffi, (1, 9, 10, 64, 8, 3, 1, 1), tile, True, 7, 120, 16, 0, 1600, fp32_kernel=True)
    _strided(ffi, (3, 14, 14, 64, 32, 1, 1, 0), tile, True, 14, 2 * 28 * 32, 2 * 32, 29 * 32, 3 * 28 * 28 * 32, fp32_kernel=True)


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("family", ["generic", "strip", "persistent", "m16_strip", "m16_persistent"])
def test_five_launches_give_the_same_bytes(ffi, family):
    """One full-chip shape per family, five launches on the same operands: identical bytes.  (Five, fixed: a check, not a stress loop.)"""
    import ctypes as C
    tile = {"generic": 10, "strip": 30, "persistent": 37, "m16_strip": 40, "m16_persistent": 47}[family]
    case = (2, 100, 168, 256, 256, 3, 1, 1)   # M = 33 600: 175 tiles of 192 rows and more of every smaller one, on 256 CUs
    ops = ref.real_operands(case)
    N, H, W, Cin, Cout, R, stride, pad = case
    d = ffi.make_conv_desc(N, H, W, Cin, Cout, R, R, stride, pad, 1, tile)
    dx = ffi.DeviceBuffer.from_numpy(ops["x"].astype(np.float16)); dw = ffi.DeviceBuffer.from_numpy(ffi.pack_conv_weights_f16(d, ops["w"]))
    ds = ffi.DeviceBuffer.from_numpy(ops["scale"]); dh = ffi.DeviceBuffer.from_numpy(ops["shift"]); dr = ffi.DeviceBuffer.from_numpy(ops["residual"].astype(np.float16))
    outs = []
    for _ in range(5):
        do = ffi.DeviceBuffer((N, H, W, Cout), np.float16).poison()
        ffi.check(ffi.lib().isegmi_op_conv2d_f16(C.byref(d), dx.ptr, dw.ptr, ds.ptr, dh.ptr, dr.ptr, do.ptr, 0, None))
        outs.append(do.numpy())
    assert not np.isnan(outs[0]).any()
    assert all(ref.same_bits(outs[0], o) for o in outs[1:])


def test_five_bottleneck_launches_give_the_same_bytes(ffi):
    rng = cc.rng_for("determinism")
    Cin, Cmid, shape = 256, 64, (2, 100, 168)
    x = np.maximum(rng.standard_normal(shape + (Cin,)), 0).astype(np.float16)
    bn = lambda c: (rng.uniform(0.5, 1.5, c).astype(np.float32), (rng.standard_normal(c) * 0.1).astype(np.float32))
    w1 = (rng.standard_normal((Cmid, 1, 1, Cin)) * (2.0 / Cin) ** 0.5).astype(np.float32)
    w2 = (rng.standard_normal((Cmid, 3, 3, Cmid)) * (2.0 / (9 * Cmid)) ** 0.5).astype(np.float32)
    w3 = (rng.standard_normal((Cin, 1, 1, Cmid)) * (2.0 / Cmid) ** 0.5).astype(np.float32)
    sb1, sb2, sb3 = bn(Cmid), bn(Cmid), bn(Cin)
    outs = [ffi.bottleneck_f16(x, w1, sb1, w2, sb2, w3, sb3) for _ in range(5)]
    assert not np.isnan(outs[0]).any() and all(ref.same_bits(outs[0], o) for o in outs[1:])
