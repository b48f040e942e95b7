"""References, error bounds and input generators for the convolution kernels: numpy only (and the seeded generator of tests/conv_cases.py) -- no GPU, no oracle, no code shared with either.

THE REFERENCE.  conv2d_fp64 is the formula: zero-pad, gather the R x S strided views into an im2col matrix, ONE fp64 matmul, then
y = scale * acc + shift (+ residual), ReLU as `y > 0 ? y : 0` (NaN -> 0, -0 -> +0: what kernels and oracle do).  Non-finite inputs are taken out of
the matmul and added back product by product, so that 0 * inf = NaN and inf - inf = NaN follow IEEE 754 whatever the BLAS does with them.

ORDER-FREE EXACT INPUTS.  exact_operands draws small integers (x in [-2, 3], w in [-2, 2] with few zeros and a per-channel sign bias, scale from
{0.5, 1, 2}, integer shift and residual).  max|x| * max|w| * K * max|scale| stays far below 2^24 (asserted), so every product, every partial sum in
ANY association -- the MFMA's internal ones included -- and the epilogue are exact in fp32 and equal the fp64 value.  The fp16 result is then the single
round-to-nearest-even of that value; expected_f16 computes it as fp64 -> fp32 -> fp16, which is no double rounding because the fp32 step is exact.
A kernel is held to it with np.array_equal on the raw bits.

THE BOUND for real-valued fp16 operands.  fp16 x fp16 products are exact in fp32 (22 significant bits, exponents far inside the fp32 range), so only
additions round.  K products summed in any order plus the three epilogue operations give
    |got - v| <= e = gamma'(K + 3) * (|scale| * abs_sum + |shift| + |residual|),   gamma'(n) = n u / (1 - n u),   abs_sum = conv(|x|, |w|).
u is taken as 2^-23, NOT 2^-24: how the MFMA adder tree rounds internally is not documented, and 2^-23 admits truncation.  This is an assumption and
not a measurement.  MEASURED on an MI355X (tests/test_conv_edges_gpu.py, every fp16 tile id x the six EDGE_CASES x both forms, 452 figures): the largest
max |got - v| / e is 0.0013, so the constant was never near and stays as derived; the CPU oracle's own ratio is 0.0001 .. 0.0035 on the same cases.

THE RMS CHECK.  e grows with abs_sum and could hide one lost product in a deep K, so on the fp32 output form rms(got - v) must not exceed
RMS_MARGIN = 2 times rms(oracle - v), the ordered fp32 chain's own error on the same operands (a blocked summation is normally more accurate than
the chain, so 2 is generous).  MEASURED on the same 452 runs: rms(got - v) / rms(oracle - v) lies between 0.35 and 0.41 for every tile family (generic,
row-strip, persistent, 16 x 16 x 32): the MFMA's blocked sums are about 2.6 times more accurate than the ordered chain.

WHICH OPS GET THE BOUND.  The single convolutions: isegmi_op_conv2d_f16 (every tile), isegmi_op_conv2d (every tile) and the fp16 stem.  The fused
kernels (bottlenecks, stem + pool, FPN merge, fused head) round an intermediate tensor to fp16, and e is not defined across that rounding: an
intermediate that lands on the other side of an fp16 tie moves every output it feeds by up to an fp16 ulp times |w|, thousands of times e.  They are
held by the zero-tolerance tests of tests/test_conv_exact_gpu.py and by the existing tests that show each of them bit-identical to the unfused launches,
which ARE under the bound; isegmi_op_conv2d_group likewise (bit-identical to its members run alone, tests/test_conv_gpu.py).
"""
import numpy as np

from conv_cases import rng_for as _rng

U = 2.0 ** -23
RMS_MARGIN = 2.0
F16_MAX = 65504.0



def h(a):
    """fp16 storage: round to nearest even, overflow -> inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(np.float16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """Equal where numbers (signed zeros told apart), NaN where NaN (any payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _im2col(x, R, S, stride, pad):
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, R, S, stride, pad)
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = np.empty((N, Ho, Wo, R, S, C), np.float64)
    for r in range(R):
        for s in range(S):
            cols[:, :, :, r, s] = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
    return cols.reshape(N * Ho * Wo, R * S * C), (N, Ho, Wo)


def conv_acc_fp64(x, w, stride=1, pad=0):
    """sum over (r, s, c) of x[n, yo * stride - pad + r, xo * stride - pad + s, c] * w[co, r, s, c] in fp64 -> [N, Ho, Wo, Cout]."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    Cout, R, S, C = w.shape
    assert x.shape[3] == C
    bad = ~np.isfinite(x)
    cols, (N, Ho, Wo) = _im2col(np.where(bad, 0.0, x), R, S, stride, pad)
    assert np.isfinite(w).all()
    acc = (cols @ w.reshape(Cout, -1).T).reshape(N, Ho, Wo, Cout)
    with np.errstate(invalid="ignore"):
        for n, y, xx, c in zip(*np.nonzero(bad)):   # IEEE by hand: each non-finite element times each weight it meets
            for r in range(R):
                for s in range(S):
                    yo, ry = divmod(y + pad - r, stride); xo, rx = divmod(xx + pad - s, stride)
                    if ry == 0 and rx == 0 and 0 <= yo < Ho and 0 <= xo < Wo:
                        acc[n, yo, xo] += x[n, y, xx, c] * w[:, r, s, c]
    return acc


def epilogue_fp64(acc, scale=None, shift=None, residual=None, act=0):
    y = np.asarray(acc, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if scale is not None:
            y = y * np.asarray(scale, np.float64)
        if shift is not None:
            y = y + np.asarray(shift, np.float64)
        if residual is not None:
            y = y + np.asarray(residual, np.float64)
        if act == 1:
            y = np.where(y > 0, y, 0.0)   # NaN -> 0 and -0 -> +0, as `y > 0 ? y : 0`
        else:
            assert act == 0
    return y


def conv2d_fp64(x, w, stride=1, pad=0, scale=None, shift=None, residual=None, act=0):
    return epilogue_fp64(conv_acc_fp64(x, w, stride, pad), scale, shift, residual, act)


def abs_sum(x, w, stride=1, pad=0):
    return conv_acc_fp64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), stride, pad)


def gamma(n, u=U):
    assert n * u < 1
    return n * u / (1.0 - n * u)


def bound(x, w, stride=1, pad=0, scale=None, shift=None, residual=None):
    """e of the module docstring, per output element."""
    Cout, R, S, C = np.shape(w)
    m = abs_sum(x, w, stride, pad)
    if scale is not None:
        m = m * np.abs(np.asarray(scale, np.float64))
    if shift is not None:
        m = m + np.abs(np.asarray(shift, np.float64))
    if residual is not None:
        m = m + np.abs(np.asarray(residual, np.float64))
    return gamma(R * S * C + 3) * m


def f16_at_or_below(v):
    """The largest fp16 value <= v (fp64 in, fp16 out; -inf below the range)."""
    v = np.asarray(v, np.float64)
    a = h(v)
    over = a.astype(np.float64) > v
    with np.errstate(over="ignore"):
        return np.where(over, np.nextafter(a, np.float16(-np.inf)), a)


def f16_at_or_above(v):
    v = np.asarray(v, np.float64)
    a = h(v)
    under = a.astype(np.float64) < v
    with np.errstate(over="ignore"):
        return np.where(under, np.nextafter(a, np.float16(np.inf)), a)


def f16_inside(got16, v, e):
    """Per element: got lies between the fp16 value just below v - e and the fp16 value just above v + e."""
    g = got16.astype(np.float64)
    return (g >= f16_at_or_below(v - e).astype(np.float64)) & (g <= f16_at_or_above(v + e).astype(np.float64))


def expected_f32(v):
    """fp64 -> fp32.  On the order-free inputs the step is exact (asserted)."""
    with np.errstate(over="ignore"):
        f = np.asarray(v).astype(np.float32)
    fin = np.isfinite(v)
    assert np.array_equal(f.astype(np.float64)[fin], np.asarray(v)[fin]), "not exactly representable in fp32"
    return f


def expected_f16(v):
    """fp64 -> fp32 (exact, asserted) -> fp16: ONE rounding, the RNE of the exact value."""
    return h(expected_f32(v))


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))


# ---------------------------------------------------------------- generators


def exact_operands(case, key=0, big_shift=False, x_lo=-2, x_hi=3):
    """Order-free exact operands of a case (N, H, W, Cin, Cout, R, stride, pad): dict of fp32 arrays x, w, scale, shift, residual, all small integers
    (scale: 0.5 / 1 / 2); x, w and residual exactly representable in fp16.  Output channel co draws its weight signs with P(+) = SIGN_BIAS[co % 6]: channels whose
    sums walk away from zero (deep K: past 2048, where the fp16 store must round) next to balanced ones.  big_shift: shifts of 2040 .. 4095."""
    N, H, W, Cin, Cout, R, stride, pad = case
    rng = _rng("exact", case, key)
    x = rng.integers(x_lo, x_hi + 1, (N, H, W, Cin)).astype(np.float32)
    mag = rng.choice(np.array([0.0, 1.0, 2.0]), (Cout, R, R, Cin), p=[1 / 16, 15 / 32, 15 / 32])
    p_plus = np.array([0.5, 0.9, 0.3, 0.7, 0.1, 0.5])[np.arange(Cout) % 6].reshape(Cout, 1, 1, 1)
    w = (mag * np.where(rng.random((Cout, R, R, Cin)) < p_plus, 1.0, -1.0)).astype(np.float32)
    scale = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), Cout)
    shift = (rng.integers(2040, 4096, Cout) if big_shift else rng.integers(-8, 9, Cout)).astype(np.float32)
    Ho, Wo = out_hw(H, W, R, R, stride, pad)
    residual = rng.integers(-4, 5, (N, Ho, Wo, Cout)).astype(np.float32)
    K = R * R * Cin
    worst = float(np.abs(x).max() * np.abs(w).max() * K * 2.0 + np.abs(shift).max() + 4)
    assert 2 * worst < 2.0 ** 24, "order-free inputs: partial sums (in halves) must stay below 2^24"
    for a in (x, w, residual):   # the fp16 tensors (scale and shift are fp32 arrays in every kernel)
        assert np.array_equal(h(a).astype(np.float32), a)
    return dict(x=x, w=w, scale=scale, shift=shift, residual=residual)


def real_operands(case, key=0):
    """Real-valued operands, fp16-representable (fp32 arrays): standard-normal x, He-scaled w, scale in [0.5, 1.5], shift ~ 0.1, normal residual."""
    N, H, W, Cin, Cout, R, stride, pad = case
    rng = _rng("real", case, key)
    x = h(rng.standard_normal((N, H, W, Cin))).astype(np.float32)
    w = h(rng.standard_normal((Cout, R, R, Cin)) * (2.0 / (R * R * Cin)) ** 0.5).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    Ho, Wo = out_hw(H, W, R, R, stride, pad)
    residual = h(rng.standard_normal((N, Ho, Wo, Cout))).astype(np.float32)
    return dict(x=x, w=w, scale=scale, shift=shift, residual=residual)


def reach(case, pixels):
    """Boolean [N, Ho, Wo]: the output positions whose R x R window contains one of `pixels` [(n, y, x), ...] (every output channel of such a position)."""
    N, H, W, Cin, Cout, R, stride, pad = case
    Ho, Wo = out_hw(H, W, R, R, stride, pad)
    m = np.zeros((N, Ho, Wo), bool)
    for (n, y, x) in pixels:
        for yo in range(Ho):
            if not 0 <= y - (yo * stride - pad) < R:
                continue
            for xo in range(Wo):
                if 0 <= x - (xo * stride - pad) < R:
                    m[n, yo, xo] = True
    return m


NONFINITE_KINDS = ["+inf", "-inf", "nan", "mixed"]


def nonfinite_operands(case, kind):
    """Order-free operands with non-finite activations at chosen pixels -> (clean operands, dirty x, reach mask).  +inf / -inf / nan: that value at a
    corner (channel 0), a border pixel (channel 63: the last of the first 64-channel chunk) and an interior pixel (channel 64 where there is one: the
    first of the next chunk; else channel 1).  mixed: +inf at the corner, -inf inside, NaN on the border."""
    N, H, W, Cin, Cout, R, stride, pad = case
    ops = exact_operands(case, key="nonfinite")
    sites = [(0, 0, 0, 0), (N - 1, H - 1, W // 2, 63), (N - 1, H // 2, W // 2, 64 if Cin > 64 else 1)]
    vals = {"+inf": [np.inf] * 3, "-inf": [-np.inf] * 3, "nan": [np.nan] * 3, "mixed": [np.inf, np.nan, -np.inf]}[kind]
    x = ops["x"].copy()
    for (n, y, xx, c), v in zip(sites, vals):
        x[n, y, xx, c] = v
    m = reach(case, [s[:3] for s in sites])
    assert m.any() and m.mean() <= 0.5, "the reachable set must leave at least half of the outputs outside"
    return ops, x, m


F16_TINY = 2.0 ** -24          # the smallest fp16 subnormal
F16_MIN_NORMAL = 2.0 ** -14
F32_MIN_NORMAL = 2.0 ** -126


def subnormal_operands(case, where):
    """Exact operands that stay exact although they are subnormal: where = 'x' (x = k * 2^-24, |k| <= 3: fp16 subnormals; w, scale normal),
    'w' (the weights are), 'both' (products k * 2^-48: normal in fp32, from two subnormal factors).  scale = 1, shift = 0, no residual: the result is
    the integer result of the unscaled operands times an exact power of two."""
    ops = exact_operands(case, key="subnormal")
    fx = F16_TINY if where in ("x", "both") else 1.0
    fw = F16_TINY if where in ("w", "both") else 1.0
    x = (ops["x"] * np.float32(fx)).astype(np.float32); w = (ops["w"] * np.float32(fw)).astype(np.float32)
    assert np.array_equal(h(x).astype(np.float32), x) and np.array_equal(h(w).astype(np.float32), w)
    return dict(x=x, w=w, scale=np.ones(case[4], np.float32), shift=np.zeros(case[4], np.float32), residual=None), fx * fw


def f32_subnormal_operands(case, where):
    """For the fp32 kernels: 'x' -> x = k * 2^-149 .. (fp32 subnormals) against integer weights: every product and sum is an exact fp32 subnormal;
    'product' -> x = k * 2^-75, w = j * 2^-74: normal factors whose products k j 2^-149 are subnormal."""
    ops = exact_operands(case, key="subnormal32")
    if where == "x":
        fx, fw = 2.0 ** -149, 1.0
    else:
        fx, fw = 2.0 ** -75, 2.0 ** -74
    x = (ops["x"].astype(np.float64) * fx).astype(np.float32); w = (ops["w"].astype(np.float64) * fw).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), ops["x"].astype(np.float64) * fx)
    return dict(x=x, w=w, scale=None, shift=None, residual=None), fx * fw


def overflow_operands(Cout):
    """A 1x1 conv over 64 channels whose exact results sit around the top of fp16: acc = 1 everywhere (x = e_0, w[:, 0] = 1), shift = target - 1.
    Targets per channel (cycled): 65504 stays, 65519 rounds down to it, 65519.996 (the last fp32 below the tie) too, the 65520 tie and everything above
    become inf; the same with the sign flipped; two ordinary values."""
    targets = np.array([65504.0, 65519.0, 65520.0 - 2.0 ** -7, 65520.0, 65536.0, 1.0e5, -65504.0, -65519.0, -65520.0, -65536.0, 1000.0, -3.0], np.float64)
    t = targets[np.arange(Cout) % len(targets)]
    x = np.zeros((2, 5, 7, 64), np.float32); x[..., 0] = 1.0
    w = np.zeros((Cout, 1, 1, 64), np.float32); w[:, 0, 0, 0] = 1.0
    shift = (t - 1.0).astype(np.float32)
    assert np.array_equal(shift.astype(np.float64), t - 1.0)
    return dict(x=x, w=w, scale=np.ones(Cout, np.float32), shift=shift, residual=None), t


def negative_zero_operands(Cout):
    """All-zero x, scale = -1, shift = -0.0: y = (+0 * -1) + -0 = -0 without ReLU (bits 0x8000), +0 with (`y > 0 ? y : 0`)."""
    x = np.zeros((1, 6, 9, 64), np.float32)
    w = exact_operands((1, 6, 9, 64, Cout, 1, 1, 0), key="negzero")["w"]
    return dict(x=x, w=w, scale=-np.ones(Cout, np.float32), shift=np.full(Cout, -0.0, np.float32), residual=None)


# ---------------------------------------------------------------- fused references (compositions, fp16 rounding where the contract rounds)
def bottleneck_fp64(x, w1, sb1, w2, sb2, w3, sb3, wd=None, sbd=None, return_inner=False):
    """Fused bottleneck: t1 = fp16(relu(bn1(conv1x1(x)))), t2 = fp16(relu(bn2(conv3x3(t1), zero padding))), out = relu(bn3(conv1x1(t2)) + shortcut),
    shortcut = x (identity) or fp16(bnd(conv1x1(x, wd))) (projection).  Returns the fp64 value before the last fp16 store."""
    t1 = h(conv2d_fp64(x, w1, 1, 0, sb1[0], sb1[1], None, 1)).astype(np.float64)
    t2 = h(conv2d_fp64(t1, w2, 1, 1, sb2[0], sb2[1], None, 1)).astype(np.float64)
    sc = np.asarray(x, np.float64) if wd is None else h(conv2d_fp64(x, wd, 1, 0, sbd[0], sbd[1], None, 0)).astype(np.float64)
    out = conv2d_fp64(t2, w3, 1, 0, sb3[0], sb3[1], sc, 1)
    return (out, t1, t2) if return_inner else out


def maxpool3x3s2_f16(x16):
    """3x3 / stride 2 / pad 1 max-pool of fp16 NHWC (exact: a max of fp16 values), -inf padding."""
    N, H, W, C = x16.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, np.float16)
    xp[:, 1:H + 1, 1:W + 1] = x16
    out = np.full((N, Ho, Wo, C), -np.inf, np.float16)
    for dr in range(3):
        for dc in range(3):
            out = np.maximum(out, xp[:, dr:dr + 2 * Ho:2, dc:dc + 2 * Wo:2])
    return out


def stem_fp64(x3, w4, scale, shift):
    """fp16 stem: the image rounded to fp16, 7x7 / 2 / pad 3 conv over its three channels (w4[..., 3] is zero by contract), BN, ReLU; fp64 out."""
    x16 = h(x3).astype(np.float64)
    return conv2d_fp64(x16, np.asarray(w4, np.float64)[..., :3], 2, 3, scale, shift, None, 1)


def merge_fp64(x, w, scale, shift, coarse):
    """lateral 1x1 + nearest-2x add: fp16(lat) + coarse[n, min(y >> 1, Hc - 1), min(x >> 1, Wc - 1)] in fp64 (the lateral is rounded to fp16 first)."""
    lat = h(conv2d_fp64(x, w, 1, 0, scale, shift, None, 0)).astype(np.float64)
    N, H, W, _ = lat.shape
    Hc, Wc = coarse.shape[1:3]
    yy = np.minimum(np.arange(H) >> 1, Hc - 1); xx = np.minimum(np.arange(W) >> 1, Wc - 1)
    return lat + np.asarray(coarse, np.float64)[:, yy][:, :, xx]


def head_fp64(x, w, scale, shift, w2, scale2, shift2):
    """3x3 + BN + ReLU rounded to fp16 (t), then the 1x1 head on t: fp32 out, no activation.  Returns (value, t)."""
    t = h(conv2d_fp64(x, w, 1, 1, scale, shift, None, 1)).astype(np.float64)
    return conv2d_fp64(t, w2, 1, 0, scale2, shift2, None, 0), t


def scatter(v, out_shape, dtype, out_div, img_stride, pix_stride, offset=0):
    """The numpy scatter of the strided output mode: element (m, co) of the [M, Cout] result goes to flat index
    offset + (m / out_div) * img_stride + (m % out_div) * pix_stride + co of an array of out_shape pre-filled with 0xFF bytes.  Returns (array, written mask)."""
    M, Cout = v.shape
    n = int(np.prod(out_shape))
    flat = np.frombuffer(b"\xff" * (n * np.dtype(dtype).itemsize), dtype).copy()
    m = np.arange(M)
    idx = (offset + (m // out_div) * img_stride + (m % out_div) * pix_stride)[:, None] + np.arange(Cout)[None, :]
    assert idx.max() < n and len(np.unique(idx)) == idx.size
    flat[idx] = v.astype(dtype)
    mask = np.zeros(n, bool); mask[idx] = True
    return flat.reshape(out_shape), mask.reshape(out_shape)


# ---------------------------------------------------------------- order-free operands of the fused kernels
def _bn_int(rng, c, scales, lo=-4, hi=4):
    return rng.choice(np.array(scales, np.float32), c), rng.integers(lo, hi + 1, c).astype(np.float32)


def _sparse_int(rng, shape, p_nonzero, mags=(1.0,)):
    return (rng.choice(np.array(mags), shape) * np.where(rng.random(shape) < 0.5, 1.0, -1.0) * (rng.random(shape) < p_nonzero)).astype(np.float32)


def bottleneck_operands(ch, shape, projection=False):
    """Integer operands of the fused bottleneck whose inner tensors t1 / t2 are exactly representable in fp16 (multiples of 1/2 below 1024; the caller
    asserts it on the reference), so the fused result has ONE right answer: x in {0, 1, 2} (a ReLU output), sparse +-1 weights in conv1 / conv2,
    scales {0.5, 1} / {1} / {0.5, 1, 2}.  -> (x, w1, sb1, w2, sb2, w3, sb3[, wd, sbd])"""
    Cin, Cmid = ch
    N, H, W = shape
    rng = _rng("bottleneck", ch, shape, projection)
    Cout = 4 * Cmid if projection else Cin
    x = rng.integers(0, 3, (N, H, W, Cin)).astype(np.float32)
    w1 = _sparse_int(rng, (Cmid, 1, 1, Cin), 0.5); sb1 = _bn_int(rng, Cmid, (0.5, 1.0))
    w2 = _sparse_int(rng, (Cmid, 3, 3, Cmid), 0.25); sb2 = _bn_int(rng, Cmid, (1.0,))
    w3 = _sparse_int(rng, (Cout, 1, 1, Cmid), 0.9, (1.0, 2.0)); sb3 = _bn_int(rng, Cout, (0.5, 1.0, 2.0))
    if not projection:
        return x, w1, sb1, w2, sb2, w3, sb3
    wd = _sparse_int(rng, (Cout, 1, 1, Cin), 0.9, (1.0, 2.0)); sbd = _bn_int(rng, Cout, (0.5, 1.0, 2.0))
    return x, w1, sb1, w2, sb2, w3, sb3, wd, sbd


def stem_operands(shape):
    """An integer image in [0, 255] (what the product feeds the stem), integer 7x7 weights in [-2, 2] over three channels (the fourth is zero by
    contract), scale 1/64 or 1/32, integer shift: the conv result is an exact multiple of 1/64 far below 2^24 / 64 and inside fp16."""
    N, H, W = shape
    rng = _rng("stem", shape)
    x = rng.integers(0, 256, (N, H, W, 3)).astype(np.float32)
    w = np.zeros((64, 7, 7, 4), np.float32)
    w[..., :3] = rng.integers(-2, 3, (64, 7, 7, 3))
    scale = rng.choice(np.array([1 / 64, 1 / 32], np.float32), 64)
    shift = rng.integers(-8, 9, 64).astype(np.float32)
    return x, w, scale, shift


def merge_operands(case):
    N, H, W, Cin, Hc, Wc = case
    ops = exact_operands((N, H, W, Cin, 256, 1, 1, 0), key="merge")
    coarse = h(_rng("coarse", case).integers(-3000, 3001, (N, Hc, Wc, 256))).astype(np.float32)   # an fp16 tensor; |sum| past 2048: half-integers that the store rounds
    return ops["x"], ops["w"], ops["scale"], ops["shift"], coarse


def head_operands(case):
    N, H, W, Cin, cout2 = case
    ops = exact_operands((N, H, W, Cin, 256, 3, 1, 1), key="head")
    rng = _rng("head2", case)
    w2 = rng.integers(-2, 3, (cout2, 1, 1, 256)).astype(np.float32)
    scale2 = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), cout2)
    shift2 = rng.integers(-8, 9, cout2).astype(np.float32)
    return ops["x"], ops["w"], ops["scale"], ops["shift"], w2, scale2, shift2


# ---------------------------------------------------------------- the expected values of the order-free cases, computed once per (case, form)
VARIANTS = [(1, True), (0, False)]   # (act, residual): residual + ReLU, and the bare conv + BN
_cache = {}


def exact_case(case, big_shift=False):
    """-> (operands, {(act, use_res): fp64 value}) of an order-free case; checked not to degenerate: at least 50 distinct values in every form and
    nothing beyond the fp16 range; K >= 2304 (or big_shift): values past 2048, where consecutive integers stop being fp16 numbers."""
    key = (case, big_shift)
    if key not in _cache:
        ops = exact_operands(case, big_shift=big_shift)
        N, H, W, Cin, Cout, R, stride, pad = case
        acc = conv_acc_fp64(ops["x"], ops["w"], stride, pad)
        vs = {}
        for act, use_res in VARIANTS:
            v = epilogue_fp64(acc, ops["scale"], ops["shift"], ops["residual"] if use_res else None, act)
            assert len(np.unique(v)) >= 50, (case, act, len(np.unique(v)))
            assert np.abs(v).max() < F16_MAX, (case, np.abs(v).max())
            if R * R * Cin >= 2304 or big_shift:
                assert (np.abs(v) > 2048).mean() > 0.01, case
                assert not np.array_equal(h(v).astype(np.float64), v), "the fp16 store must have something to round"
            vs[(act, use_res)] = v
        _cache[key] = (ops, vs)
    return _cache[key]
