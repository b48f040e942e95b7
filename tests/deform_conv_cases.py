"""Cases and references of the fused deformable convolution (TEST INFRASTRUCTURE ONLY).  The operator reference is the oracle's unfused form:
ora.deform_im2col, then ora.conv2d as a 1x1 over the 9 C column channels (scale, shift, residual, act).  The unmodulated form (18 offset channels) is fed to
the oracle as the 18 offsets plus nine mask logits of +100: dm_sigmoid gives exactly 1.0 there and v * 1.0 is exact (tests/test_oracle_cpu.py relies on a
saturated mask the same way; test_deform_conv_cpu.py asserts it).  `sample_np` restates the sampling rule in numpy, one rounded fp32 operation per step, with
switches for the WRONG rules the CPU tests tell apart.  Everything here is computed from seeds, once per process, and never modified."""
import functools

import numpy as np

from oracle import ora

TILE = 64          # output pixels per block of deform_conv_kernel (DC_TP in csrc/deform_conv.hip)
BAND = 64          # output channels per block: Cout 4 / 32 sit below it, 96 is a band and a half, 260 / 516 four / eight bands and a 4-channel rest
SAT = np.float32(100.0)   # a saturated mask logit: dm_sigmoid(100) == 1.0


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def as27(om):
    """18 offset channels -> the oracle's 27 (saturated logits); 27 pass through."""
    om = np.asarray(om, np.float32)
    if om.shape[-1] == 27:
        return om
    assert om.shape[-1] == 18, om.shape
    return np.concatenate([om, np.full(om.shape[:-1] + (9,), SAT, np.float32)], -1)


def columns(x, om, stride):
    return ora.deform_im2col(x, as27(om), 3, 3, stride, 1, 1)


def reference(x, om, w, stride=1, scale=None, shift=None, residual=None, act=0):
    """-> (output [N, Ho, Wo, Cout], columns [N, Ho, Wo, 9 C]) of the oracle's two-step form."""
    col = columns(x, om, stride)
    cout = w.shape[0]
    return ora.conv2d(col, np.ascontiguousarray(w, np.float32).reshape(cout, 1, 1, -1), 1, 0, scale, shift, residual, act), col


def base_positions(H, W, stride):
    """-> (bh, bw) [Ho, Wo, 9] float32: the undeformed sampling position of every (output pixel, tap)."""
    Ho, Wo = out_hw(H, W, stride)
    k = np.arange(9)
    bh = (np.arange(Ho)[:, None, None] * stride - 1 + (k // 3)[None, None, :]) + np.zeros((1, Wo, 1), np.int64)
    bw = (np.arange(Wo)[None, :, None] * stride - 1 + (k % 3)[None, None, :]) + np.zeros((Ho, 1, 1), np.int64)
    return bh.astype(np.float32), bw.astype(np.float32)


def positions(om, H, W, stride):
    """-> (h, w) [N, Ho, Wo, 9] float32, as the kernels compute them: (float) base + offset, one rounded add."""
    om = np.asarray(om, np.float32)
    bh, bw = base_positions(H, W, stride)
    with np.errstate(invalid="ignore"):
        return bh[None] + om[..., 0:18:2], bw[None] + om[..., 1:18:2]


def dead_rows(om, H, W, stride):
    """Number of (pixel, tap) positions outside (-1, H) x (-1, W) -- computed from the geometry alone (NaN compares false, so it is dead)."""
    h, w = positions(om, H, W, stride)
    with np.errstate(invalid="ignore"):
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    return int((~inside).sum())


def zero_rows(col, C):
    """Number of all-zero (pixel, tap) rows of a column tensor."""
    return int((col.reshape(-1, C) == 0).all(-1).sum())


def sample_np(x, om, stride, swap_yx=False, ignore_mask=False, mask_at_2k=False, ge_border=False):
    """The sampling rule restated in numpy (each operation a rounded fp32 one): -> columns [N, Ho, Wo, 9 C].  With no switch set it equals
    ora.deform_im2col bit for bit (asserted by the CPU tests); each switch is one WRONG rule."""
    x = np.asarray(x, np.float32); om = as27(om)
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, stride)
    dy, dx = om[..., 0:18:2], om[..., 1:18:2]
    if swap_yx:
        dy, dx = dx, dy
    logit = om[..., 0:18:2] if mask_at_2k else om[..., 18:27]
    m = np.ones_like(logit) if ignore_mask else ora.map_f32(np.ascontiguousarray(logit), 1)
    bh, bw = base_positions(H, W, stride)
    F = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        h, w = bh[None] + dy, bw[None] + dx
        inside = ((h >= -1) if ge_border else (h > -1)) & ((w >= -1) if ge_border else (w > -1)) & (h < H) & (w < W)
        hs, ws = np.where(inside, h, F(0)), np.where(inside, w, F(0))
        hf, wf = np.floor(hs), np.floor(ws)
        hl, wl = hf.astype(np.int64), wf.astype(np.int64)
        lh, lw = hs - hf, ws - wf
        hh, hw = F(1) - lh, F(1) - lw
        w1, w2, w3, w4 = hh * hw, hh * lw, lh * hw, lh * lw
        n = np.arange(N)[:, None, None, None]

        def corner(hi, wi):
            ok = (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            v = x[n, np.clip(hi, 0, H - 1), np.clip(wi, 0, W - 1)]   # [N, Ho, Wo, 9, C]
            return np.where(ok[..., None], v, F(0))
        v1, v2, v3, v4 = corner(hl, wl), corner(hl, wl + 1), corner(hl + 1, wl), corner(hl + 1, wl + 1)
        v = ((w1[..., None] * v1 + w2[..., None] * v2) + w3[..., None] * v3) + w4[..., None] * v4
        v = (v * m[..., None]).astype(np.float32)
        v = np.where(inside[..., None], v, F(0))
    return np.ascontiguousarray(v.reshape(N, Ho, Wo, 9 * C), np.float32)


# ---- seeded random cases ------------------------------------------------------------------------------------------------------------------------------
def random_case(seed, N, H, W, C, Cout, stride, modulated, res_relu):
    """Offsets of about +-1.5 pixels (some taps leave a small image), mask logits around 0, features in [0.5, 1.5] (no all-zero row inside the image)."""
    rng = np.random.default_rng([seed, N, H, W, C, Cout, stride, int(modulated), int(res_relu)])
    Ho, Wo = out_hw(H, W, stride)
    x = rng.uniform(0.5, 1.5, (N, H, W, C)).astype(np.float32)
    om = rng.normal(0, 1.5, (N, Ho, Wo, 27 if modulated else 18)).astype(np.float32)
    w = (rng.standard_normal((Cout, 3, 3, C)) / np.sqrt(9.0 * C)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.5, Cout).astype(np.float32)
    residual = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32) if res_relu else None
    return dict(x=x, om=om, w=w, stride=stride, scale=scale, shift=shift, residual=residual, act=1 if res_relu else 0)


def _tile_hw(pixels):
    """One image whose output pixel count is `pixels` (stride 1): 1 x pixels."""
    return 1, 1, pixels


# (N, H, W, C, Cout, stride, modulated, res_relu): every value of every axis the issue lists appears, and the axes that share code paths are crossed --
# the three image sizes with both strides and both forms; the pixel counts TILE - 1, TILE, TILE + 1; every C with a Cout; every Cout (and 516: eight bands and a rest).
RANDOM_SHAPES = (
    [(n, h, w, 32, 32, s, m, r) for (n, h, w) in ((1, 1, 1), (1, 5, 7), (2, 9, 13)) for s in (1, 2) for (m, r) in ((1, 1), (0, 0))] +
    [_tile_hw(p) + (32, 32, 1, m, r) for p in (TILE - 1, TILE, TILE + 1) for (m, r) in ((1, 0), (0, 1))] +
    [(2, 9, 13, c, co, s, m, r) for (c, co, s, m, r) in ((64, 4, 1, 1, 1), (160, 96, 2, 0, 1), (256, 260, 1, 1, 0), (160, 32, 1, 0, 0), (64, 96, 2, 1, 0),
                                                       (256, 4, 2, 0, 1), (32, 260, 2, 1, 1), (32, 516, 1, 0, 1), (64, 260, 1, 0, 0), (160, 4, 1, 1, 0))])


@functools.lru_cache(maxsize=None)
def random_reference(i):
    c = random_case(20261020, *RANDOM_SHAPES[i])
    ref, col = reference(c["x"], c["om"], c["w"], c["stride"], c["scale"], c["shift"], c["residual"], c["act"])
    for a in list(c.values()) + [ref, col]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, ref, col


# ---- crafted offsets ----------------------------------------------------------------------------------------------------------------------------------
CH, CW, CC, CCOUT = 5, 7, 32, 32   # the crafted cases' image, channels and outputs (stride 1: 35 output pixels, 315 (pixel, tap) rows)
CRAFTED = ("integer", "on_minus1_and_H", "last_row_col", "between_minus1_and_0", "huge", "nonfinite", "one_pixel_all_out")


def _aim(om, target_h, target_w, stride=1):
    """Offsets that put EVERY (pixel, tap) exactly on (target_h, target_w) [broadcastable to Ho, Wo, 9]: the differences are exact in fp32."""
    bh, bw = base_positions(CH, CW, stride)
    om[0, ..., 0:18:2] = np.float32(target_h) - bh
    om[0, ..., 1:18:2] = np.float32(target_w) - bw


@functools.lru_cache(maxsize=None)
def crafted(kind, modulated):
    """-> (case dict, reference output, reference columns, expected number of all-zero (pixel, tap) rows)."""
    rng = np.random.default_rng([77, CRAFTED.index(kind), int(modulated)])
    x = rng.uniform(0.5, 1.5, (1, CH, CW, CC)).astype(np.float32)
    om = np.zeros((1, CH, CW, 27 if modulated else 18), np.float32)
    if modulated:
        om[..., 18:] = rng.normal(0, 1.0, (1, CH, CW, 9))
    k = np.arange(9)
    rows = CH * CW * 9
    if kind == "integer":            # integer positions, some of them outside: tap k of pixel (ho, wo) lands on (ho + k - 4, wo + 4 - k)
        bh, bw = base_positions(CH, CW, 1)
        th = np.arange(CH)[:, None, None] + (k - 4)[None, None, :] + np.zeros((1, CW, 1), np.int64)
        tw = np.arange(CW)[None, :, None] + (4 - k)[None, None, :] + np.zeros((CH, 1, 1), np.int64)
        _aim(om, th, tw)
        want = int(((th < 0) | (th > CH - 1) | (tw < 0) | (tw > CW - 1)).sum())
        assert 0 < want < rows
    elif kind == "on_minus1_and_H":  # exactly on h = -1 (even taps) and on h = H (odd taps): the comparisons are strict, every row is dead
        _aim(om, np.where(k % 2 == 0, -1.0, float(CH))[None, None, :], 2.0)
        want = rows
    elif kind == "last_row_col":     # exactly on h = H - 1, w = W - 1: only corner 1 is inside the image, with weight 1
        _aim(om, float(CH - 1), float(CW - 1))
        want = 0
    elif kind == "between_minus1_and_0":   # h in (-1, 0): the two upper corners are outside
        _aim(om, -0.5, 2.25)
        want = 0
    elif kind == "huge":             # +-1e6: far outside, every row dead
        om[..., 0:18:2] = np.where(k % 2 == 0, 1e6, -1e6)
        om[..., 1:18:2] = np.where(k % 3 == 0, -1e6, 1e6)
        want = rows
    elif kind == "nonfinite":        # +-inf and NaN sample zero through the comparison; taps 0-2 keep a finite in-range position
        om[..., 0:18:2] = np.asarray([0, 0, 0, np.inf, -np.inf, np.nan, 0, 0, np.nan], np.float32)
        om[..., 1:18:2] = np.asarray([0, 0, 0, 0, 0, 0, np.inf, np.nan, -np.inf], np.float32)
        want = CH * CW * 6 + 3 * CW + 2 * (CH - 1)   # taps 3-8 everywhere; taps 0-2 of the first row (h = -1); tap 0 at wo = 0 and tap 2 at wo = W - 1
    else:                            # one pixel (2, 3) with all nine taps outside, the others random: its output is shift (+ act)
        om[..., :18] = rng.normal(0, 0.7, (1, CH, CW, 18))
        om[0, 2, 3, 0:18:2] = -50.0
        want = dead_rows(om, CH, CW, 1)
        assert want >= 9
    assert dead_rows(om, CH, CW, 1) == want, (kind, dead_rows(om, CH, CW, 1), want)
    w = (rng.standard_normal((CCOUT, 3, 3, CC)) / np.sqrt(9.0 * CC)).astype(np.float32)
    shift = rng.normal(0, 0.5, CCOUT).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, CCOUT).astype(np.float32)
    c = dict(x=x, om=om, w=w, stride=1, scale=scale, shift=shift, residual=None, act=1)
    ref, col = reference(x, om, w, 1, scale, shift, None, 1)
    for a in (x, om, w, shift, scale, ref, col):
        a.setflags(write=False)
    return c, ref, col, want


@functools.lru_cache(maxsize=None)
def nonfinite_features(modulated):
    """Integer positions (zero offsets): the bilinear weights of corners 2-4 are exactly 0, and 0 * inf = NaN reaches the sample wherever one of those
    corners holds a non-finite feature.  x has +inf, -inf and NaN pixels; the reference decides what comes out."""
    rng = np.random.default_rng([78, int(modulated)])
    x = rng.uniform(0.5, 1.5, (1, CH, CW, CC)).astype(np.float32)
    x[0, 1, 2, :] = np.inf; x[0, 3, 4, 5] = -np.inf; x[0, 4, 6, 7] = np.nan
    om = np.zeros((1, CH, CW, 27 if modulated else 18), np.float32)
    w = (rng.standard_normal((CCOUT, 3, 3, CC)) / np.sqrt(9.0 * CC)).astype(np.float32)
    c = dict(x=x, om=om, w=w, stride=1, scale=None, shift=None, residual=None, act=0)
    ref, col = reference(x, om, w, 1)
    assert np.isnan(col).any() and np.isfinite(col).any()
    return c, ref, col
