"""The conv kernels on ORDER-FREE EXACT inputs (tests/conv_ref.py): small integers whose every product and partial sum is exact in fp32 in any
association, so the result does not depend on how a kernel, or the MFMA inside it, orders its additions.  It has ONE right answer -- the fp64 value,
rounded once to fp16 where the output is fp16 -- and every comparison below is np.array_equal on the raw bits against a reference that shares no code
with the kernels (one fp64 matmul; held to the CPU oracle and to torch in tests/test_conv_ref_cpu.py).  Random integer weights make a swapped, dropped
or doubled tap, chunk, row or column change the answer.  No tolerance anywhere in this file."""
import numpy as np
import pytest

import conv_cases as cc
import conv_ref as ref

pytestmark = pytest.mark.gpu


def _diff(got, want):
    bad = ref.bits(got) != ref.bits(want)
    idx = np.argwhere(bad)
    return "%d of %d differ; first at %s: got %r, want %r" % (int(bad.sum()), bad.size, idx[0].tolist() if len(idx) else None,
                                                              got[tuple(idx[0])] if len(idx) else None, want[tuple(idx[0])] if len(idx) else None)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(ref.bits(got), ref.bits(want)), "%s: %s" % (what, _diff(got, want))


def _run_f16(ffi, case, tile, ops, vs, forms):
    for act, use_res, f32 in forms:
        v = vs[(act, use_res)]
        got = ffi.conv2d_f16(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"] if use_res else None, act, tile, out_f32=f32)
        _same(got, ref.expected_f32(v) if f32 else ref.expected_f16(v), "tile %d act %d res %d f32 %d" % (tile, act, use_res, f32))


ALL_FORMS = [(act, use_res, f32) for (act, use_res) in ref.VARIANTS for f32 in (False, True)]


@pytest.mark.parametrize("case", cc.EXACT_CASES)
@pytest.mark.parametrize("tile", cc.F16_TILES)
def test_conv_f16_exact(ffi, case, tile):
    """isegmi_op_conv2d_f16, every tile id of the launcher: fp16 and fp32 outputs, with residual + ReLU and without.  A pair the launcher's ARG_CHECK
    refuses (conv_cases.f16_refused: the one rule) must be refused, with an error and not a launch."""
    ops, vs = ref.exact_case(case)
    if cc.f16_refused(tile, case):
        with pytest.raises(ffi.IsegmiError):
            ffi.conv2d_f16(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], None, 0, tile)
        return
    _run_f16(ffi, case, tile, ops, vs, ALL_FORMS)


@pytest.mark.parametrize("tile", cc.F16_TILES)
def test_conv_f16_exact_where_the_store_rounds(ffi, tile):
    """A shallow case with integer shifts of 2040 .. 4095: results are half-integers past 2048, so the fp16 store rounds (ties included)."""
    ran = 0
    for case in (cc.BIG_SHIFT_CASE, cc.BIG_SHIFT_CASE_3X3):
        if cc.f16_refused(tile, case):
            continue
        ops, vs = ref.exact_case(case, big_shift=True)
        _run_f16(ffi, case, tile, ops, vs, ALL_FORMS)
        ran += 1
    assert ran


@pytest.mark.parametrize("tile", cc.F16_TILES)
def test_conv_f16_exact_around_the_tile_height(ffi, tile):
    """M = BM - 1, BM, BM + 1 for every BM of the tile table (64 .. 256): the last tile full, one row short, one row over."""
    for M in cc.BM_EDGES:
        case = cc.bm_edge_case(M)
        ops, vs = ref.exact_case(case)
        _run_f16(ffi, case, tile, ops, vs, [(1, True, False), (0, False, True)])


@pytest.mark.parametrize("case", cc.F32_CASES)
@pytest.mark.parametrize("tile", cc.F32_TILES)
def test_conv_f32_exact(ffi, case, tile):
    """isegmi_op_conv2d (fp32) on the same kind of inputs against the same kind of expected values: every tile of test_conv_bit_exact, and 15 -- the
    fixed-tree split-K, whose tree an exact sum does not care about."""
    ops, vs = ref.exact_case(case)
    for (act, use_res), v in vs.items():
        got = ffi.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"] if use_res else None, act, tile)
        _same(got, ref.expected_f32(v), "tile %d act %d res %d" % (tile, act, use_res))


@pytest.mark.parametrize("case", cc.F32_HYBRID_CASES)
@pytest.mark.parametrize("tile", [13, 14])
def test_conv_f32_hybrid_exact(ffi, case, tile):
    """Tiles 13 / 14 where the launch really splits into 64 x 64 tiles and 32 x 32 blocks."""
    ops, vs = ref.exact_case(case)
    got = ffi.conv2d(ops["x"], ops["w"], case[6], case[7], ops["scale"], ops["shift"], ops["residual"], 1, tile)
    _same(got, ref.expected_f32(vs[(1, True)]))


def test_conv_group_exact(ffi):
    """isegmi_op_conv2d_group: members that differ in everything, one launch, each against its own fp64 value."""
    cases = [cc.F32_CASES[i] for i in (0, 2, 4, 8, 9)] + [cc.F32_HYBRID_CASES[1]]
    items, wants = [], []
    for i, case in enumerate(cases):
        ops, vs = ref.exact_case(case)
        act, use_res = ref.VARIANTS[i % 2]
        items.append(dict(x=ops["x"], w=ops["w"], stride=case[6], pad=case[7], act=act, scale=ops["scale"], shift=ops["shift"],
                          residual=ops["residual"] if use_res else None))
        wants.append(ref.expected_f32(vs[(act, use_res)]))
    for got, want, case in zip(ffi.conv2d_group(items), wants, cases):
        _same(got, want, str(case))


# ---------------------------------------------------------------- the fp16 stem
_stem_cache = {}


def _stem(shape):
    if shape not in _stem_cache:
        x, w, scale, shift = ref.stem_operands(shape)
        e16 = ref.expected_f16(ref.stem_fp64(x, w, scale, shift))
        assert np.isfinite(e16).all() and len(np.unique(e16)) >= 50
        _stem_cache[shape] = (x, w, scale, shift, e16, ref.maxpool3x3s2_f16(e16))
    return _stem_cache[shape]


@pytest.mark.parametrize("shape", cc.STEM_SHAPES)
@pytest.mark.parametrize("tile", [0, 8])
def test_stem_f16_exact(ffi, shape, tile):
    x, w, scale, shift, e16, _ = _stem(shape)
    got, halo = ffi.stem_f16(x, w, scale, shift, tile)
    _same(got, e16)


@pytest.mark.parametrize("shape", cc.STEM_SHAPES)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_stem_pool_f16_exact(ffi, shape, flags):
    """The fused stem + max-pool under every flags value a release build accepts (bit 0: blocks walk many units; bit 1: the shortest units)."""
    x, w, scale, shift, _, pooled = _stem(shape)
    _same(ffi.stem_pool_f16(x, w, scale, shift, flags), pooled)


# ---------------------------------------------------------------- the fused bottleneck
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("shape", cc.BOTTLENECK_SHAPES)
@pytest.mark.parametrize("ch", cc.BOTTLENECK_CH)
def test_bottleneck_f16_exact(ffi, ch, shape, flags):
    """t1 and t2 are exactly representable (asserted on the reference), so rounding them to fp16 changes nothing and the fused result has one right answer."""
    ops = ref.bottleneck_operands(ch, shape)
    out, t1, t2 = ref.bottleneck_fp64(*ops, return_inner=True)
    x, w1, sb1, w2, sb2 = ops[:5]
    assert np.array_equal(t1, ref.conv2d_fp64(x, w1, 1, 0, sb1[0], sb1[1], None, 1)) and np.array_equal(t2, ref.conv2d_fp64(t1, w2, 1, 1, sb2[0], sb2[1], None, 1))
    assert max(t1.max(), t2.max()) < 2048 and len(np.unique(out)) >= 50 and out.max() < ref.F16_MAX
    _same(ffi.bottleneck_f16(*ops, flags=flags), ref.expected_f16(out))


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("shape", cc.BOTTLENECK_SHAPES)
def test_bottleneck_ds_f16_exact(ffi, shape, flags):
    ops = ref.bottleneck_operands((64, 64), shape, projection=True)
    out, t1, t2 = ref.bottleneck_fp64(*ops, return_inner=True)
    assert max(t1.max(), t2.max()) < 2048 and len(np.unique(out)) >= 50 and out.max() < ref.F16_MAX
    assert np.array_equal(t2, ref.conv2d_fp64(t1, ops[3], 1, 1, ops[4][0], ops[4][1], None, 1))
    _same(ffi.bottleneck_ds_f16(*ops, flags=flags), ref.expected_f16(out))


def test_bottleneck_f16_pads_t1_with_zero(ffi):
    """All-zero x and a positive bn1 shift: t1 = relu(shift) inside the image, 0 in conv2's padding (tests/test_conv_ref_cpu.py shows that the border
    outputs then differ from the interior ones).  A t1 halo holding relu(shift) fails here."""
    for ch, shape in (((256, 64), (1, 6, 7)), ((512, 128), (2, 19, 37))):
        x, w1, sb1, w2, sb2, w3, sb3 = ref.bottleneck_operands(ch, shape)
        x = np.zeros_like(x); sb1 = (sb1[0], np.abs(sb1[1]) + 1.0); w2 = np.abs(w2) * (np.arange(w2.shape[0]).reshape(-1, 1, 1, 1) % 3 < 2)
        out, t1, t2 = ref.bottleneck_fp64(x, w1, sb1, w2, sb2, w3, sb3, return_inner=True)
        assert (t1 > 0).all() and max(t1.max(), t2.max()) < 2048 and not np.array_equal(t2[:, 0, 0], t2[:, 2, 3])
        for flags in (0, 1):
            _same(ffi.bottleneck_f16(x, w1, sb1, w2, sb2, w3, sb3, flags=flags), ref.expected_f16(out))


# ---------------------------------------------------------------- the fused FPN merge and RPN head, under every MFMA shape setting
def _under_every_mfma_shape(ffi, run):
    assert ffi.get_f16_mfma_shape() == 3
    outs = []
    for shape in (0, 1, 2, 3):
        ffi.set_f16_mfma_shape(shape)
        try:
            outs.append(run())
        finally:
            ffi.set_f16_mfma_shape(3)
    return outs


@pytest.mark.parametrize("case", cc.MERGE_CASES)
def test_conv1x1_up2x_add_f16_exact(ffi, case):
    """Lateral 1x1 + nearest-2x add.  Setting 2 runs the merge on v_mfma_f32_16x16x32_f16 (tile 48 of conv_f16_m16_launch), the others on the 32 x 32 x 16
    persistent tile.  Odd H / W: the last row / column reads coarse[min(y >> 1, Hc - 1)]; Hc, Wc one below and far above half the size."""
    x, w, scale, shift, coarse = ref.merge_operands(case)
    want = ref.expected_f16(ref.merge_fp64(x, w, scale, shift, coarse))
    assert np.isfinite(want).all()
    for i, got in enumerate(_under_every_mfma_shape(ffi, lambda: ffi.conv1x1_up2x_add_f16(x, w, scale, shift, coarse))):
        _same(got, want, "mfma shape %d" % i)


@pytest.mark.parametrize("case", cc.HEAD_CASES)
def test_conv3x3_head_f16_exact(ffi, case):
    """3x3 + BN + ReLU (t, rounded to fp16) with the fused 1x1 head, fp32 out.  Setting 0 runs it on the 32 x 32 x 16 row-strip tile (30), 1 - 3 on tile 40."""
    x, w, scale, shift, w2, scale2, shift2 = ref.head_operands(case)
    v, t = ref.head_fp64(x, w, scale, shift, w2, scale2, shift2)
    want = ref.expected_f32(v)
    assert len(np.unique(want)) >= 50 and (t > 2048).any() == (case[3] >= 256)
    for i, (got, fused) in enumerate(_under_every_mfma_shape(ffi, lambda: ffi.conv3x3_head_f16(x, w, scale, shift, w2, scale2, shift2))):
        assert fused, "half a round of 192-row tiles: the launcher fuses"
        _same(got, want, "mfma shape %d" % i)
