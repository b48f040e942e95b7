"""Plain references for the HBM-bound spatial ops (csrc/spatial.hip, csrc/spatial_f16.hip) and the small R-CNN tails next to them, written
from the formulas and not from the kernels, plus the error bounds that say how far an fp32 evaluation may land from the fp64 ones.  Test
infrastructure only: numpy, no GPU, no oracle.

    maxpool                 np.pad with -inf, then the max over the k x k strided views of the padded map: exact (for inputs free of NaN; the
                            sign of a zero result is that of np.maximum, so callers keep mixed-sign zeros out of what they compare here)
    nearest2x_add           lateral + coarse[min(y >> 1, Hc - 1), min(x >> 1, Wc - 1)], one IEEE addition in the dtype handed in: exact
    resize_bilinear         F.interpolate(bilinear, align_corners = False) in fp64: src = max((dst + 0.5) in / out - 0.5, 0), taps floor(src) and
                            the next one (clamped to the map), weights 1 - frac and frac; + add; ReLU
    avgpool_full            fp64 mean over the window
    mask_logits_select      1 / (1 + exp(-(x @ w[label] + b[label]))) in fp64, zeros for label <= 0
    grid_anchors            base[a] + (x, y, x, y) * stride at row (y * grid_w + x) * A + a; the shifts are small integers, the one fp32 addition
                            is numpy's: exact
    pad_c3_to_c4            a zero 4th channel: exact

Error bounds (u = 2^-24, the fp32 unit roundoff; gamma(n) = n u / (1 - n u), so that a product of n factors (1 + e_i), |e_i| <= u, is within
gamma(n) of 1).

mask tail.  An fp32 sum of the C products x_c w_c and the bias in which every term passes through at most n roundings (an FMA rounds once) is
    |z_hat - z| <= gamma(n) (sum_c |x_c w_c| + |b|),
whatever the association.  The sequential chain (the fp32 kernel, the generic fp16 kernel, the oracle) has n = C + 1: C chained FMAs and the
bias FMA.  The C = 256 fp16 kernel has n = 14: 8 chained FMAs per lane, 5 butterfly additions over the 32 lanes, the bias FMA.  The logistic
function has slope <= 1/4, and the project's dm_sigmoid is within 1.5e-7 of the fp64 one on [-30, 30] (the figure asserted by
tests/test_oracle_cpu.py::test_detmath_accuracy; mask_logits_select refuses logits outside that range).  Hence
    |out - ref| <= 0.25 gamma(n) (sum_c |x_c w_c| + |b|) + 1.5e-7          per pixel, from the inputs at hand.

bilinear resize.  Per axis the fp32 coordinate is src_hat = fl(fl(fl(in / out) (dst + 0.5)) - 0.5); dst + 0.5 is exact and
(in / out) (dst + 0.5) < in, so the three roundings give |src_hat - src| <= gamma(3) in.  The clamp at 0 does not increase that.  As a function
of the position the interpolant of the edge-replicated map is continuous and piecewise linear with slope at most D, the largest difference
between neighbouring samples along that axis (taken here over the whole map of that image and channel), so that moving the position costs at
most Dx gamma(3) W + Dy gamma(3) H -- also when floor(src_hat) and floor(src) differ.  The weights: frac = src_hat - floor(src_hat) is exact
(Sterbenz), 1 - frac is rounded once (<= u).  With M the largest |sample| of that image and channel, top = fma(lx1, v01, fl(lx0 v00)) is within
u M (the weight) + u M (the product) + u M (the FMA) = 3u M of its exact value, bot likewise, and v = fma(ly1, bot, fl(ly0 top)) adds
ly0 3u M + ly1 3u M + u M (the weight 1 - ly1) + u M + u M: 6u M + O(u^2 M), taken as 7u M.  Together
    B0 = gamma(3) (W Dx + H Dy) + 7u M.
The optional addition rounds once more, u (|v + add| + B0); ReLU is exact and does not expand distances.  An fp16 store adds half an fp16 ulp of
the stored value (f16_store_slack).  Nothing here is fitted to an implementation: tests/test_spatial_ref_cpu.py holds the CPU oracle to
these bounds at every shape the GPU tests use.

avgpool_full.  A sequential fp32 sum of HW terms, then one division by the exact float HW:
    |got - mean| <= gamma(HW - 1) sum |x| / HW + u |mean|.
(the cross term u gamma(HW - 1) sum |x| / HW of the division is inside gamma's over-estimate of (1 + u)^(HW - 1) - 1: k^2 >= k (k + 1) / 2.)"""
import numpy as np

U = 2.0 ** -24
SIGMOID_ERR = 1.5e-7        # tests/test_oracle_cpu.py::test_detmath_accuracy
SIGMOID_RANGE = 30.0        # the interval that figure was taken on


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------- exact references
def maxpool_out_hw(H, W, k, s, p):
    """Output size; (0, 0) when the padded map is smaller than the window (nothing to pool)."""
    if H + 2 * p < k or W + 2 * p < k:
        return 0, 0
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def maxpool(x, k, s, p):
    """x [N, H, W, C] of any float dtype, free of NaN -> [N, Ho, Wo, C] of the same dtype."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = maxpool_out_hw(H, W, k, s, p)
    assert Ho > 0 and Wo > 0 and not np.isnan(x).any()
    P = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)), constant_values=-np.inf)
    out = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    for r in range(k):
        for q in range(k):
            out = np.maximum(out, P[:, r:r + s * (Ho - 1) + 1:s, q:q + s * (Wo - 1) + 1:s, :])
    return out


def nearest2x_add(coarse, lateral):
    """coarse [N, Hc, Wc, C], lateral [N, H, W, C], same dtype -> lateral + nearest-2x(coarse) in that dtype."""
    coarse = np.asarray(coarse); lateral = np.asarray(lateral)
    assert coarse.dtype == lateral.dtype
    _, Hc, Wc, _ = coarse.shape
    _, H, W, _ = lateral.shape
    yi = np.minimum(np.arange(H) >> 1, Hc - 1)
    xi = np.minimum(np.arange(W) >> 1, Wc - 1)
    with np.errstate(over="ignore"):
        return lateral + coarse[:, yi][:, :, xi]


def grid_anchors(base, stride, grid_h, grid_w):
    base = np.asarray(base, np.float32)
    yy, xx = np.indices((grid_h, grid_w))
    shift = (np.stack([xx, yy, xx, yy], axis=-1) * int(stride)).astype(np.float32)
    out = shift[:, :, None, :] + base[None, None, :, :]
    return out.reshape(-1, 4)


def pad_c3_to_c4(x):
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape[:-1] + (4,), np.float32)
    out[..., :3] = x
    return out


# ---------------------------------------------------------------- fp64 references and their bounds
def _axis(in_sz, out_sz):
    src = np.maximum((np.arange(out_sz, dtype=np.float64) + 0.5) * (in_sz / out_sz) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_sz - 1)
    i1 = np.minimum(i0 + 1, in_sz - 1)
    return i0, i1, src - i0


def resize_bilinear(x, Ho, Wo, add=None, relu=False):
    """-> (ref fp64 [N, Ho, Wo, C], bound [N, Ho, Wo, C]) for an fp32 evaluation stored as fp32 (module docstring)."""
    x = np.asarray(x, np.float64)
    N, H, W, C = x.shape
    y0, y1, fy = _axis(H, Ho)
    x0, x1, fx = _axis(W, Wo)
    fy = fy[None, :, None, None]; fx = fx[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = r0[:, :, x0] * (1 - fx) + r0[:, :, x1] * fx
    bot = r1[:, :, x0] * (1 - fx) + r1[:, :, x1] * fx
    v = top * (1 - fy) + bot * fy
    Dy = np.abs(np.diff(x, axis=1)).max(axis=(1, 2), keepdims=True) if H > 1 else np.zeros((N, 1, 1, C))
    Dx = np.abs(np.diff(x, axis=2)).max(axis=(1, 2), keepdims=True) if W > 1 else np.zeros((N, 1, 1, C))
    M = np.abs(x).max(axis=(1, 2), keepdims=True)
    bound = np.broadcast_to(gamma(3) * (W * Dx + H * Dy) + 7 * U * M, v.shape).copy()
    if add is not None:
        v = v + np.asarray(add, np.float64)
        bound = bound + U * (np.abs(v) + bound)
    if relu:
        v = np.maximum(v, 0.0)
    return v, bound


def f16_store_slack(ref, bound):
    """Half an fp16 ulp of whatever is stored: the value lies within `bound` of `ref`; 2^-11 relative in the normal range, 2^-25 below it."""
    return np.maximum((np.abs(ref) + bound) * 2.0 ** -11, 2.0 ** -25)


def avgpool_full(x):
    """x [R, H, W, C] -> (mean fp64 [R, C], bound [R, C])"""
    x = np.asarray(x, np.float64)
    R, H, W, C = x.shape
    HW = H * W
    mean = x.reshape(R, HW, C).mean(axis=1)
    bound = gamma(HW - 1) * np.abs(x).reshape(R, HW, C).sum(axis=1) / HW + U * np.abs(mean)
    return mean, bound


def mask_logits_select(feat, w, b, labels, depth, rows=64):
    """feat [R, HW, C]; w [ncls, C]; b [ncls]; labels [R]; depth = the roundings a term passes through (C + 1 for the chain, 14 for the C = 256
    fp16 kernel) -> (ref fp64 [R, HW], bound [R, HW]); rows with label <= 0 are 0 with bound 0.  Evaluated `rows` rows at a time."""
    R, HW, C = feat.shape
    w = np.asarray(w, np.float64); b = np.asarray(b, np.float64)
    ref = np.zeros((R, HW)); bound = np.zeros((R, HW))
    for r0 in range(0, R, rows):
        lab = np.asarray(labels[r0:r0 + rows])
        on = lab >= 1
        if not on.any():
            continue
        x = np.asarray(feat[r0:r0 + rows][on], np.float64)
        wl = w[lab[on]][:, None, :]; bl = b[lab[on]][:, None]
        z = (x * wl).sum(axis=2) + bl
        assert np.abs(z).max() < SIGMOID_RANGE, "logits outside the range the sigmoid figure was taken on"
        mag = (np.abs(x) * np.abs(wl)).sum(axis=2) + np.abs(bl)
        idx = r0 + np.nonzero(on)[0]
        ref[idx] = 1.0 / (1.0 + np.exp(-z))
        bound[idx] = 0.25 * gamma(depth) * mag + SIGMOID_ERR
    return ref, bound
