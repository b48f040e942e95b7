"""The shapes and seeded inputs shared by tests/test_spatial_f16_gpu.py, tests/test_spatial_gpu.py (kernel against oracle and reference) and
tests/test_spatial_ref_cpu.py (oracle against reference at the very same shapes and inputs).  The shapes ARE the point: every list below names
what its members are there to hit."""
import zlib

import numpy as np

F16_MAX = 65504.0


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def h(x):
    """fp16 storage: round to fp16 (overflow -> inf)."""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- max-pool
MAXPOOL_KSP = [(3, 2, 1), (1, 2, 0), (2, 2, 0), (3, 1, 1)]
# (N, H, W): odd / even, H = 1, W = 1, W = 2, 1 x 1, and two sizes whose (H + 2p - k) is not a multiple of s
MAXPOOL_NHW = [(2, 19, 23), (1, 16, 24), (2, 1, 9), (2, 9, 1), (1, 7, 2), (3, 1, 1), (1, 2, 2), (1, 10, 13)]
MAXPOOL_F16_FORMS = [("c8", True, 8), ("c8", True, 64), ("c8", True, 256), ("quad", True, 4), ("quad", True, 12), ("quad", True, 68),
                     ("float", False, 4), ("float", False, 64)]
MAXPOOL_F32_C = [4, 12, 32, 256]
# the models' own: the stem's conv output of a 800 x 1344 canvas (N = 1), and P5 -> P6 of the same canvas
MAXPOOL_MODEL = [((1, 400, 672, 64), (3, 2, 1)), ((1, 25, 42, 256), (1, 2, 0))]
# more than 4096 x 256 = 1 048 576 work items of 8 channels (2 x 200 x 336 x 8 = 1 075 200), not a multiple of it
MAXPOOL_GRID_STRIDE = ((2, 400, 672, 64), (3, 2, 1))

_SPECIAL_ALL = [np.inf, -np.inf, np.nan, 0.0, -0.0, F16_MAX, -F16_MAX, 2.0 ** -24, -2.0 ** -24, 3.0e-5, -3.0e-5]
_SPECIAL_CLEAN = [np.inf, -np.inf, 0.0, F16_MAX, -F16_MAX, 2.0 ** -24, -2.0 ** -24, 3.0e-5, -3.0e-5]
# fp32 input of the float form: values that round to fp16 on the way out (to inf, to 65504, to a subnormal, to zero, ties)
_SPECIAL_F32 = [1.0e5, -1.0e5, 65520.0, 65519.0, 1.0e-8, -1.0e-8, 2.0 ** -25, 3.0 * 2.0 ** -25, 1.00048828125, 3.4e38, 1.0e-40]


def maxpool_out_hw(H, W, k, s, p):
    if H + 2 * p < k or W + 2 * p < k:
        return 0, 0
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def maxpool_input(shape, dtype, clean, key):
    """Normal data pushed below zero (so that a window's maximum is often one of its zeros), a quarter of the elements replaced by special values
    -- borders, interiors and neighbours alike -- and the four corners forced to specials.  clean: no NaN and no -0 (what the index-arithmetic
    reference may be compared on)."""
    rng = rng_for("maxpool", shape, np.dtype(dtype).name, clean, key)
    N, H, W, C = shape
    x = rng.standard_normal(shape) - 1.0
    sp = list(_SPECIAL_CLEAN if clean else _SPECIAL_ALL)
    if np.dtype(dtype) == np.float32:
        sp += _SPECIAL_F32
    sp = np.array(sp)
    pick = sp[rng.integers(0, len(sp), shape)]
    x = np.where(rng.random(shape) < 0.25, pick, x)
    for (yy, xx) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        x[:, yy, xx, :] = sp[(np.arange(C) + yy + xx) % len(sp)]
    with np.errstate(over="ignore"):
        x = x.astype(dtype)
    if clean:
        x = np.where(x == 0, np.zeros((), dtype), x)   # a value that underflowed to -0
    return x


def maxpool_cases_small(C):
    for nhw in MAXPOOL_NHW:
        for ksp in MAXPOOL_KSP:
            ho, wo = maxpool_out_hw(nhw[1], nhw[2], *ksp)
            if ho > 0 and wo > 0:
                yield nhw + (C,), ksp


# ---------------------------------------------------------------- nearest 2x + add
NEAREST_C = [4, 12, 256]
NEAREST_F32_C = [4, 12, 32, 256]
NEAREST_N = [1, 3]
# P2-sized map with 64 channels at N = 2: 2 x 200 x 336 x 64 / 4 = 2 150 400 work items
NEAREST_GRID_STRIDE = (2, 100, 168, 64, 200, 336)


def nearest_geometries():
    """(Hc, Wc, H, W): H in {2 Hc, 2 Hc - 1, 2 Hc + 1} and the same for W (the clamp); Hc = 1."""
    for Hc, Wc in ((5, 7), (1, 3)):
        for H in (2 * Hc, 2 * Hc - 1, 2 * Hc + 1):
            for W in (2 * Wc, 2 * Wc - 1, 2 * Wc + 1):
                yield Hc, Wc, H, W


def nearest_input(N, Hc, Wc, C, H, W, dtype, key=0):
    """Data whose sums mostly are not numbers of `dtype` (the addition rounds); pairs of +-big whose sum overflows to +-inf (60000 in fp16, 3e38 in
    fp32); lateral = -coarse where it lands (x + (-x) = +0)."""
    rng = rng_for("nearest", N, Hc, Wc, C, H, W, np.dtype(dtype).name, key)
    big = np.asarray(60000.0 if np.dtype(dtype) == np.float16 else 3.0e38, dtype)
    coarse = (rng.standard_normal((N, Hc, Wc, C)) * 3.0).astype(dtype)
    lateral = (rng.standard_normal((N, H, W, C)) * 0.37).astype(dtype)
    yi = np.minimum(np.arange(H) >> 1, Hc - 1); xi = np.minimum(np.arange(W) >> 1, Wc - 1)
    coarse = np.where(rng.random(coarse.shape) < 0.1, np.where(rng.random(coarse.shape) < 0.5, big, -big), coarse).astype(dtype)
    up = coarse[:, yi][:, :, xi]
    m = rng.random(lateral.shape)
    lateral = np.where(m < 0.1, -up, lateral)                                                  # cancels exactly
    lateral = np.where((m >= 0.1) & (m < 0.3) & (np.abs(up) == big), up, lateral)              # overflows
    return coarse, lateral.astype(dtype)


# ---------------------------------------------------------------- bilinear resize
# (N, H, W, C, Ho, Wo): Yolact's own chains (18 -> 35 -> 69 feed an add, 69 -> 138 and 35 -> 70 a ReLU; every case runs all four
# add / relu combinations), identity, a downscale, 1 x 1 input, 1-wide output, C in {4, 32, 256}
RESIZE_CASES = [(1, 18, 18, 256, 35, 35), (1, 35, 35, 256, 69, 69), (1, 69, 69, 256, 138, 138), (1, 35, 35, 256, 70, 70),
                (2, 9, 11, 32, 9, 11), (2, 20, 30, 32, 7, 11), (2, 1, 1, 4, 5, 6), (2, 6, 9, 4, 4, 1), (1, 19, 23, 32, 38, 46),
                (3, 5, 1, 4, 3, 8)]
RESIZE_F32_CASES = RESIZE_CASES + [(2, 19, 23, 12, 35, 41)]
RESIZE_GRID_STRIDE = (2, 100, 168, 64, 200, 336)      # 2 150 400 work items


def resize_input(case, dtype, key=0):
    N, H, W, C, Ho, Wo = case
    rng = rng_for("resize", case, np.dtype(dtype).name, key)
    x = (rng.standard_normal((N, H, W, C)) * 2.0).astype(dtype)
    add = (rng.standard_normal((N, Ho, Wo, C)) * 0.7).astype(dtype)
    return x, add


# ---------------------------------------------------------------- mask tail
MASK_NCLS = 7
MASK_GENERIC_C = [4, 64, 128, 260]
MASK_GENERIC_HW = [1, 49, 300]          # 300: a thread's second pixel
MASK_C256_HW = [784, 196, 1, 2, 7, 8, 9, 31, 32, 33, 785]
MASK_C256_R = [1, 37, 800]
MASK_F32_HW = [1, 196, 784, 785]
MASK_F32_C = [4, 256, 1024]


def mask_labels(R, rng, with_empty):
    lab = rng.integers(1, MASK_NCLS, R).astype(np.int32)
    if with_empty and R >= 3:
        lab[1::5] = 0
        lab[2::7] = -1
    return lab


def mask_weights(C, key=0):
    rng = rng_for("mask_w", C, key)
    w = (rng.standard_normal((MASK_NCLS, C)) / np.sqrt(C)).astype(np.float32)
    b = (rng.standard_normal(MASK_NCLS) * 0.5).astype(np.float32)
    return w, b


def mask_feat(R, HW, C, dtype, key=0, rows=64):
    rng = rng_for("mask_x", R, HW, C, np.dtype(dtype).name, key)
    out = np.empty((R, HW, C), dtype)
    for r0 in range(0, R, rows):
        n = min(rows, R - r0)
        out[r0:r0 + n] = rng.standard_normal((n, HW, C), dtype=np.float32) * 1.5
    return out


def mask_c256_kernel_association(feat16, w, b, labels):
    """The C = 256 fp16 kernel's order restated in numpy fp32: lane l chains channels 8 l .. 8 l + 7 from +0 (the FMA is formed in fp64, where the product of
    an fp16 and an fp32 number is exact, and rounded to fp32), the 32 partial sums are added pairwise at distances 16, 8, 4, 2, 1, then the bias.  Rows
    with label >= 1 only; returns the fp32 logits [R, HW] (NaN elsewhere)."""
    R, HW, C = feat16.shape
    assert C == 256
    z = np.full((R, HW), np.nan, np.float32)
    on = np.nonzero(np.asarray(labels) >= 1)[0]
    for r in on:
        x = feat16[r].astype(np.float64).reshape(HW, 32, 8)
        wl = w[labels[r]].astype(np.float64).reshape(1, 32, 8)
        acc = np.zeros((HW, 32), np.float32)
        for i in range(8):
            acc = (x[:, :, i] * wl[:, :, i] + acc.astype(np.float64)).astype(np.float32)
        d = 16
        while d >= 1:
            acc = acc + acc[:, np.arange(32) ^ d]
            d >>= 1
        z[r] = (acc[:, 0].astype(np.float64) + np.float64(b[labels[r]])).astype(np.float32)
    return z


# ---------------------------------------------------------------- the rest of the fp32 sweep
AVGPOOL_CASES = [(1, 1, 1, 4), (37, 7, 7, 64), (300, 7, 7, 2048), (3, 14, 14, 12)]     # (R, HW, C) = (1, 1, 4), (37, 49, 64), (300, 49, 2048), (3, 196, 12)
ANCHOR_A = [1, 3, 15]
ANCHOR_STRIDES = [4, 8, 16, 32, 64]
ANCHOR_GRIDS = [(1, 1), (1, 7), (200, 336)]
PAD_NPIX = [1, 255, 257, 800 * 1344 * 2]


def anchor_base(A, stride):
    rng = rng_for("anchors", A, stride)
    half = np.round(rng.uniform(2, 8, (A, 2)) * stride * 2) / 4       # quarter-pixel sizes, like the rounded base anchors
    c = (stride - 1) / 2.0
    return np.concatenate([c - half, c + half], axis=1).astype(np.float32)


def grid_stride_tail(total_items, per_item, cap_items):
    """Flat element range of the work items past the last whole sweep of a grid capped at cap_items threads."""
    assert total_items > cap_items and total_items % cap_items
    return (total_items // cap_items) * cap_items * per_item, total_items * per_item
