"""A second, independent restatement of Pose2Seg's pose-specific stages in fp64, written from the formulas and not
from any operation order, plus the error bounds that say how far an fp32 implementation of them may land from it.  Test infrastructure
only: it imports neither tests/pose2seg_ref.py nor the oracle.

    letterbox   bilinear sample (zeros outside, integer pixel centres) of the image at m1^-1 (x, y, 1), then the u8 rounding, the ImageNet
                normalisation
    fit         per template np.linalg.lstsq on the sqrt(w)-scaled rows; error = sum w |r|^2 / sum w; argmin, ties to the lowest t; the
                stated fallback.  A keypoint with a non-finite coordinate is not visible.
    align       theta = inv(A H A^-1) (np.linalg.inv), affine_grid's base grid, grid_sample's unnormalise, bilinear with zeros -- evaluated
                per pixel, never folded into one matrix
    skeleton    Gaussian heatmaps exp(-d^2 / (2 sigma^2)) cut where the exponent passes 4.6052, limb unit vectors on the band |perp| < 1 of
                the window [max(rint(min - 1), 0), min(rint(max + 1), 64))
    masks       softmax, sampled at H m2 m1 (x, y, 1), > 0.5, the tight box (right / bottom exclusive)

Error bounds (u = 2^-24, the fp32 unit roundoff).  An fp32 warp computes s = (g0 x + g1 y) + g2 from fp32 g; against the exact fp64
position it is off by at most  ds = 4u (|g0 x| + |g1 y| + |g2|) + 2u |s|  (rounding of the three matrix entries, two products and two sums).
A bilinear sample moves by at most D (|dsx| + |dsy|) when its position moves, D the largest difference between neighbouring taps of the
cells around it (the zero padding included), and the fp32 mix itself adds at most 12u max|tap| (the weights 1 - w and six rounded
operations); both are zero where no fp32 operation rounds (exact matrices and positions, short fractions).  Everything after that is a handful of correctly rounded fp32 operations, each u relative.  A thresholded output (u8
rounding, > 0.5, the limb band, the heatmap cut, the template argmin) must match exactly unless the fp64 value lies within its bound of the
threshold: that is the "ambiguous" set, which the checks count and keep under 0.5 % of the elements."""
import numpy as np

U = 2.0 ** -24
S_IN, S_FEAT, S_ALIGN = 512, 128, 64
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SIGMA = 3.0
HEAT_CUT = 4.6052          # exp(-4.6052) ~ 0.01
MAX_AMBIGUOUS = 0.005

KEYPOINTS = ["nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
             "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle"]
SKELETON = [("left_ankle", "left_knee"), ("left_knee", "left_hip"), ("right_ankle", "right_knee"), ("right_knee", "right_hip"),
            ("left_hip", "right_hip"), ("left_shoulder", "left_hip"), ("right_shoulder", "right_hip"), ("left_shoulder", "right_shoulder"),
            ("left_shoulder", "left_elbow"), ("right_shoulder", "right_elbow"), ("left_elbow", "left_wrist"), ("right_elbow", "right_wrist"),
            ("left_eye", "right_eye"), ("nose", "left_eye"), ("nose", "right_eye"), ("left_eye", "left_ear"), ("right_eye", "right_ear"),
            ("left_ear", "left_shoulder"), ("right_ear", "right_shoulder")]   # the COCO person skeleton
LIMBS = [(KEYPOINTS.index(a), KEYPOINTS.index(b)) for a, b in SKELETON]


def m1_matrix(h, w):
    s = min(S_IN / w, S_IN / h)
    return np.array([[s, 0.0, S_IN / 2 - s * w / 2], [0.0, s, S_IN / 2 - s * h / 2], [0.0, 0.0, 1.0]])


M2 = np.diag([S_FEAT / S_IN, S_FEAT / S_IN, 1.0])


# ---------------------------------------------------------------- bilinear sampling with zero padding, and its sensitivity
def _pixels(h, w):
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return x, y


def bilinear(img, sx, sy):
    """img [H, W, C]; sx / sy fp64 positions -> (values [..., C] fp64, D [...]: the largest neighbouring-tap step around each sample)"""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    P = np.pad(img, ((2, 2), (2, 2), (0, 0)))
    inside = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)          # NaN positions are outside
    x0 = np.floor(np.where(inside, sx, 0)).astype(np.int64)
    y0 = np.floor(np.where(inside, sy, 0)).astype(np.int64)
    fx = np.where(inside, sx, 0) - x0
    fy = np.where(inside, sy, 0) - y0
    t = lambda dy, dx: P[y0 + 2 + dy, x0 + 2 + dx]
    e = lambda a: a[..., None]
    v = (t(0, 0) * e((1 - fx) * (1 - fy)) + t(0, 1) * e(fx * (1 - fy)) + t(1, 0) * e((1 - fx) * fy) + t(1, 1) * e(fx * fy))
    v = np.where(e(inside), v, 0.0)
    g = np.zeros(P.shape[:2])
    g[:, :-1] = np.abs(np.diff(P, axis=1)).max(2)
    g[:-1, :] = np.maximum(g[:-1, :], np.abs(np.diff(P, axis=0)).max(2))
    win = np.zeros((H + 1, W + 1))
    for dy in range(4):
        for dx in range(4):
            win = np.maximum(win, g[dy:dy + H + 1, dx:dx + W + 1])
    fxc = np.clip(np.floor(np.nan_to_num(sx, nan=-1.0, posinf=W, neginf=-1)), -1, W - 1).astype(np.int64)
    fyc = np.clip(np.floor(np.nan_to_num(sy, nan=-1.0, posinf=H, neginf=-1)), -1, H - 1).astype(np.int64)
    return v, win[fyc + 1, fxc + 1]


def _is_f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64) == a


def position_error(g6, x, y):
    """the bound on |fp32 (g0 x + g1 y) + g2 - exact| for both rows of a 2 x 3 matrix (fp64 g, rounded to fp32 by the implementation).
    Zero where every entry, product and sum is an fp32 number: then no operation rounds."""
    g = np.asarray(g6, np.float64).reshape(-1)
    out = []
    for r in (0, 3):
        a, b, c = g[r] * x, g[r + 1] * y, g[r + 2]
        exact = _is_f32(g[r]) & _is_f32(g[r + 1]) & _is_f32(c) & _is_f32(a) & _is_f32(b) & _is_f32(a + b) & _is_f32(a + b + c)
        out.append(np.where(exact, 0.0, 4 * U * (np.abs(a) + np.abs(b) + abs(c)) + 2 * U * np.abs(a + b + c)))
    return out


def _mix_error(sx, sy, dx, dy, tap_max):
    """the fp32 bilinear mix's own rounding: none when the position is exact and both fractions are multiples of 2^-7 (with integer taps
    below 2^8 every product and sum then needs at most 8 + 1 + 7 + 7 + 1 = 24 bits), else 12u max|tap|"""
    short = lambda s: (s * 2.0 ** 7) == np.floor(s * 2.0 ** 7)
    with np.errstate(invalid="ignore"):
        exact = (dx == 0) & (dy == 0) & short(sx) & short(sy) & (tap_max < 256) & (tap_max == np.floor(tap_max))
    return np.where(exact, 0.0, 12 * U * tap_max)


class Ambiguity:
    """counts the elements a check could not decide (fp64 value within its bound of a threshold)"""

    def __init__(self):
        self.amb, self.total = 0, 0

    def add(self, amb_mask):
        self.amb += int(np.count_nonzero(amb_mask)); self.total += int(np.size(amb_mask))
        return amb_mask

    def check(self):
        assert self.total > 0 and self.amb <= MAX_AMBIGUOUS * self.total, "ambiguous %d of %d" % (self.amb, self.total)


# ---------------------------------------------------------------- 1. letterbox
def letterbox(img_u8, swap_rb=0):
    """-> (v [512, 512, 3]: the warped pixel before rounding, in output channel order; its error bound [512, 512])"""
    h, w = img_u8.shape[:2]
    r = max(w, h) / S_IN                      # 1 / s, exact: m1^-1 in closed form keeps the samples that land on a pixel or a half exact
    minv = np.array([[r, 0.0, w / 2 - r * S_IN / 2], [0.0, r, h / 2 - r * S_IN / 2]])
    x, y = _pixels(S_IN, S_IN)
    sx = minv[0, 0] * x + minv[0, 1] * y + minv[0, 2]
    sy = minv[1, 0] * x + minv[1, 1] * y + minv[1, 2]
    v, D = bilinear(img_u8, sx, sy)
    if swap_rb:
        v = v[..., ::-1]
    dx, dy = position_error(minv, x, y)
    return v, D * (dx + dy) + _mix_error(sx, sy, dx, dy, 255.0)


def normalise(v):
    return (v / 255.0 - np.asarray(MEAN)) / np.asarray(STD)


def check_letterbox(got, img_u8, swap_rb, round_u8, amb=None):
    """got [512, 512, 4] fp32 (the kernel's or the restatement's plane)"""
    got = np.asarray(got, np.float64)
    assert not got[..., 3].any()
    v, bv = letterbox(img_u8, swap_rb)
    if not round_u8:
        want = normalise(v)
        tol = bv[..., None] / (255.0 * np.asarray(STD)) + 8 * U * (np.abs(want) + 3.0)
        err = np.abs(got[..., :3] - want)
        assert np.all(err <= tol), float((err - tol).max())
        return
    level = np.clip(np.floor(v + 0.5), 0, 255)
    got_level = (got[..., :3] * np.asarray(STD) + np.asarray(MEAN)) * 255.0
    assert np.all(np.abs(got_level - np.rint(got_level)) < 1e-3)      # the kernel's output is a normalised integer level
    frac = np.abs(v + 0.5 - np.rint(v + 0.5))                          # distance to the nearest rounding boundary k + 0.5
    a = (frac <= bv[..., None]) & (bv[..., None] > 0)               # a zero bound: the implementation computes v exactly
    amb = amb or Ambiguity()
    amb.add(a)
    bad = (np.rint(got_level) != level) & ~a
    assert not bad.any(), (np.argwhere(bad)[:5], v[bad][:5])
    return amb


# ---------------------------------------------------------------- 2. fit
def fit(kpts, m1, templates, align_corners=0):
    """kpts [17, 3] image pixels, m1 3 x 3, templates [T, 17, 3] -> dict(H 3 x 3, t (-1: fallback), err, errs, runner_up, rel (the
    relative error bound of H), G / Mmask 2 x 3, kalign [17, 3])"""
    k = np.asarray(kpts, np.float64)
    vis = np.isfinite(k[:, 0]) & np.isfinite(k[:, 1]) & (k[:, 2] > 0)
    kf = np.zeros((17, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        m21 = M2 @ m1
        kf[vis] = (m21[:2, :2] @ k[vis, :2].T).T + m21[:2, 2]
    tp = np.asarray(templates, np.float64)
    errs, fits, conds, margins = [], [], [], []
    for t in range(tp.shape[0]):
        use = vis & (tp[t, :, 2] > 0)
        w = tp[t, use, 2]
        P = np.stack([kf[use, 0], kf[use, 1], np.ones(use.sum())], 1)
        if use.sum() < 3:
            errs.append(np.inf); fits.append(None); conds.append(1.0); margins.append(np.inf)
            continue
        S = P.T @ (P * w[:, None])
        det, tr = np.linalg.det(S), np.trace(S)
        margins.append(abs(abs(det) - 1e-9 * tr ** 3) / (1e-9 * tr ** 3))
        if not abs(det) > 1e-9 * tr ** 3:
            errs.append(np.inf); fits.append(None); conds.append(1.0)
            continue
        sw = np.sqrt(w)[:, None]
        X = np.linalg.lstsq(P * sw, tp[t, use, :2] * sw, rcond=None)[0]     # [3, 2]: column c maps (x, y, 1) to template coordinate c
        r = P @ X - tp[t, use, :2]
        errs.append(float((w * (r ** 2).sum(1)).sum() / w.sum()))
        fits.append(X.T)
        conds.append(np.linalg.cond(S))
    errs = np.array(errs)
    if np.isfinite(errs).any():
        t = int(np.argmin(errs))                    # the first minimum: ties to the lowest t
        H = np.vstack([fits[t], [0.0, 0.0, 1.0]])
        rest = [errs[u] for u in range(len(errs)) if u != t and not np.array_equal(tp[u], tp[t])]   # a duplicate of t ties exactly on both sides
        runner = float(min(rest)) if rest else np.inf
        rel = 64 * conds[t] * 2.0 ** -53
    else:
        t, runner, rel = -1, np.inf, 16 * 2.0 ** -53
        if vis.any():
            x0, y0 = kf[vis].min(0); x1, y1 = kf[vis].max(0)
            side = max(max(x1 - x0, y1 - y0) * 1.2, 8.0)
            s = S_ALIGN / side
            H = np.array([[s, 0.0, S_ALIGN / 2 - s * (x0 + x1) / 2], [0.0, s, S_ALIGN / 2 - s * (y0 + y1) / 2], [0.0, 0.0, 1.0]])
        else:
            H = np.diag([S_ALIGN / S_FEAT, S_ALIGN / S_FEAT, 1.0])
    kal = np.zeros((17, 3))
    kal[:, :2] = (H[:2, :2] @ kf.T).T + H[:2, 2]
    kal[:, 2] = np.where(np.isfinite(k[:, 0]) & np.isfinite(k[:, 1]), k[:, 2], 0.0)
    return dict(H=H, t=t, err=float(errs[t]) if t >= 0 else 0.0, errs=errs, runner_up=runner, rel=rel, det_margin=min(margins) if margins else np.inf,
                G=align_positions_matrix(H, align_corners), Mmask=(H @ M2 @ m1)[:2], kalign=kal, m21=M2 @ m1)


def check_fit(got_m3, got_G, got_mmask, got_kal, got_t, want):
    """the kernel's outputs of one instance against fit(); returns False when the template choice is ambiguous (nothing else is checked)"""
    if want["det_margin"] < 1e-6:
        return False
    if want["t"] >= 0 and want["runner_up"] - want["err"] <= 1e-7 * want["err"] + want["rel"] * 1e4:
        return False
    assert got_t == want["t"], (got_t, want["t"], want["errs"])
    H, rel = want["H"], want["rel"]
    scale = np.abs(H[:2]).sum(1, keepdims=True)
    assert np.all(np.abs(np.asarray(got_m3, np.float64).reshape(2, 3) - H[:2]) <= (rel + 2 * U) * scale), (got_m3, H)
    for got, M in ((got_G, want["G"]), (got_mmask, want["Mmask"])):
        sc = np.abs(M).sum(1, keepdims=True) + 1.0
        tol = (4 * U + 1e3 * rel) * sc
        assert np.all(np.abs(np.asarray(got, np.float64).reshape(2, 3) - M) <= tol), (got, M)
    k = want["kalign"]
    vis = k[:, 2] > 0
    g = np.asarray(got_kal, np.float64)
    assert np.array_equal(g[:, 2], k[:, 2])
    tol = (2 * U + 1e3 * rel) * (np.abs(k[vis, :2]) + 64.0)
    assert np.all(np.abs(g[vis, :2] - k[vis, :2]) <= tol)
    return True


# ---------------------------------------------------------------- 3. Affine-Align, from affine_grid + grid_sample's formulas
def align_positions(H, align_corners, n=S_ALIGN):
    """the P2 pixel position every align-frame pixel samples: theta = inv(A H A^-1) on affine_grid's base grid over 128 x 128, grid_sample's
    unnormalise to the 128 x 128 map, the top-left n x n crop"""
    A = np.array([[2.0 / S_FEAT, 0.0, -1.0], [0.0, 2.0 / S_FEAT, -1.0], [0.0, 0.0, 1.0]])
    theta = np.linalg.inv(A @ np.asarray(H, np.float64) @ np.linalg.inv(A))
    x, y = _pixels(n, n)
    if align_corners:
        bx, by = 2.0 * x / (S_FEAT - 1) - 1.0, 2.0 * y / (S_FEAT - 1) - 1.0
    else:
        bx, by = (2.0 * x + 1.0) / S_FEAT - 1.0, (2.0 * y + 1.0) / S_FEAT - 1.0
    gx = theta[0, 0] * bx + theta[0, 1] * by + theta[0, 2]
    gy = theta[1, 0] * bx + theta[1, 1] * by + theta[1, 2]
    if align_corners:
        return (gx + 1.0) / 2.0 * (S_FEAT - 1), (gy + 1.0) / 2.0 * (S_FEAT - 1)
    return ((gx + 1.0) * S_FEAT - 1.0) / 2.0, ((gy + 1.0) * S_FEAT - 1.0) / 2.0


def align_positions_matrix(H, align_corners):
    """the affine map of align_positions read off at three pixels (for comparing an implementation's matrix)"""
    sx, sy = align_positions(H, align_corners, 2)
    return np.array([[sx[0, 1] - sx[0, 0], sx[1, 0] - sx[0, 0], sx[0, 0]], [sy[0, 1] - sy[0, 0], sy[1, 0] - sy[0, 0], sy[0, 0]]])


def check_align(got, feat, H, align_corners):
    """got [64, 64, C]; feat [Hf, Wf, C]; the implementation samples at an fp32 rounding of the positions' affine map"""
    sx, sy = align_positions(H, align_corners)
    want, D = bilinear(feat, sx, sy)
    x, y = _pixels(S_ALIGN, S_ALIGN)
    dx, dy = position_error(align_positions_matrix(H, align_corners), x, y)
    tol = D * (dx + dy) + 12 * U * np.abs(feat).max() + 1e-30
    err = np.abs(np.asarray(got, np.float64) - want).max(-1)
    assert np.all(err <= tol), (float((err / tol).max()), np.unravel_index(np.argmax(err / tol), err.shape))


# ---------------------------------------------------------------- 4. skeleton
def skeleton(kal):
    """kal [17, 3] align-frame keypoints -> [64, 64, 55]: 17 heatmaps, then (ux, uy) of every limb on its band"""
    kal = np.asarray(kal, np.float64)
    x, y = _pixels(S_ALIGN, S_ALIGN)
    out = np.zeros((S_ALIGN, S_ALIGN, 55))
    for j in range(17):
        if kal[j, 2] > 0:
            e = ((x - kal[j, 0]) ** 2 + (y - kal[j, 1]) ** 2) / (2 * SIGMA * SIGMA)
            out[..., j] = np.where(e <= HEAT_CUT, np.exp(-e), 0.0)
    for l, (a, b) in enumerate(LIMBS):
        (ax, ay, va), (bx, by, vb) = kal[a], kal[b]
        norm = np.hypot(bx - ax, by - ay)
        if not (va > 0 and vb > 0 and norm > 0):
            continue
        ux, uy = (bx - ax) / norm, (by - ay) / norm
        win = ((x >= max(np.rint(min(ax, bx) - 1), 0)) & (x < min(np.rint(max(ax, bx) + 1), S_ALIGN))
               & (y >= max(np.rint(min(ay, by) - 1), 0)) & (y < min(np.rint(max(ay, by) + 1), S_ALIGN)))
        on = win & (np.abs((x - ax) * uy - (y - ay) * ux) < 1.0)
        out[..., 17 + 2 * l] = np.where(on, ux, 0.0)
        out[..., 18 + 2 * l] = np.where(on, uy, 0.0)
    return out


def check_skeleton(got, kal, amb=None):
    """got [64, 64, >= 55] (channels past 55 must be zero); kal [17, 3] the fp32 align-frame keypoints the implementation was given"""
    got = np.asarray(got, np.float64)
    kal = np.asarray(kal, np.float32).astype(np.float64)
    amb = amb or Ambiguity()
    assert not got[..., 55:].any()
    x, y = _pixels(S_ALIGN, S_ALIGN)
    for j in range(17):
        g = got[..., j]
        if not kal[j, 2] > 0:
            assert not g.any(), j
            continue
        e = ((x - kal[j, 0]) ** 2 + (y - kal[j, 1]) ** 2) / (2 * SIGMA * SIGMA)
        de = 12 * U * e + 4 * U * (np.abs(x - kal[j, 0]) + np.abs(y - kal[j, 1])) ** 2 / (2 * SIGMA * SIGMA)
        a = amb.add(np.abs(e - HEAT_CUT) <= de + 4 * U * HEAT_CUT)
        on = (e <= HEAT_CUT) & ~a
        off = (e > HEAT_CUT) & ~a
        want = np.exp(-e)
        assert not g[off].any(), j
        assert np.all(np.abs(g[on] - want[on]) <= want[on] * (de[on] + 8 * U)), (j, float(np.abs(g[on] - want[on]).max()))
    for l, (a_, b_) in enumerate(LIMBS):
        gx, gy = got[..., 17 + 2 * l], got[..., 18 + 2 * l]
        ax, ay, bx, by = kal[a_, 0], kal[a_, 1], kal[b_, 0], kal[b_, 1]
        norm = np.hypot(bx - ax, by - ay)
        if not (kal[a_, 2] > 0 and kal[b_, 2] > 0) or not norm > 0:
            assert not gx.any() and not gy.any(), l
            continue
        ux, uy = (bx - ax) / norm, (by - ay) / norm
        win = np.ones((S_ALIGN, S_ALIGN), bool)
        wamb = np.zeros((S_ALIGN, S_ALIGN), bool)
        for c, (p, q) in ((x, (ax, bx)), (y, (ay, by))):
            lo, hi = min(p, q) - 1.0, max(p, q) + 1.0
            win &= (c >= max(np.rint(lo), 0.0)) & (c < min(np.rint(hi), float(S_ALIGN)))
            for edge in (lo, hi):       # an end of the window rounds from fp32 (v -/+ 1): ambiguous when that lands on a half
                if abs(edge - np.floor(edge) - 0.5) <= 4 * U * (abs(edge) + 1.0):
                    wamb |= np.abs(c - edge) <= 1.0
        perp = (x - ax) * uy - (y - ay) * ux
        dp = 16 * U * (np.abs(x - ax) + np.abs(y - ay)) + 4 * U
        a = amb.add(wamb | (win & (np.abs(np.abs(perp) - 1.0) <= dp)))
        on = win & (np.abs(perp) < 1.0) & ~a
        off = ~(win & (np.abs(perp) < 1.0)) & ~a
        assert not gx[off].any() and not gy[off].any(), l
        assert np.all(np.abs(gx[on] - ux) <= 8 * U) and np.all(np.abs(gy[on] - uy) <= 8 * U), l
    return amb


# ---------------------------------------------------------------- 5. masks
def softmax_fg(logits):
    """channel 1 of the 2-way softmax, fp64"""
    l = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.maximum(l[..., 0], l[..., 1])
        e0, e1 = np.exp(l[..., 0] - m), np.exp(l[..., 1] - m)
        return e1 / (e0 + e1)


def check_mask(got_mask, got_box, logits, mmask6, h, w, amb=None, extra=0.0):
    """got_mask [h, w] u8, got_box xyxy; logits [64, 64, 2]; mmask6 the (fp32) matrix the implementation used; `extra`: a further bound on
    the implementation's probabilities (when its logits are not these)"""
    amb = amb or Ambiguity()
    M = np.asarray(mmask6, np.float64).reshape(2, 3)
    x, y = _pixels(h, w)
    sx = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    sy = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    p, D = bilinear(softmax_fg(logits)[..., None], sx, sy)
    p = p[..., 0]
    dx, dy = position_error(M, x, y)
    bound = D * (dx + dy) + 12 * U + 16 * U + extra      # the move, the mix, the softmax (two exps, a sum, a divide)
    a = amb.add(np.abs(p - 0.5) <= bound)
    want = p > 0.5
    got = np.asarray(got_mask).astype(bool)
    assert got.shape == (h, w)
    bad = (got != want) & ~a
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:3])
    sure, maybe = want & ~a, want | a
    box = np.asarray(got_box, np.float64)
    if not got.any():
        assert not sure.any() and not box.any()
        return amb
    ys, xs = np.nonzero(got)
    assert list(box) == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]   # the box is the tight box of the mask it came with
    if sure.any():
        ys, xs = np.nonzero(sure)
        assert box[0] <= xs.min() and box[1] <= ys.min() and box[2] >= xs.max() + 1 and box[3] >= ys.max() + 1
    ys, xs = np.nonzero(maybe)
    assert box[0] >= xs.min() and box[1] >= ys.min() and box[2] <= xs.max() + 1 and box[3] <= ys.max() + 1
    return amb


# ---------------------------------------------------------------- inputs
def smooth_image(rng, h, w, cycles=1.5):
    """uint8 [h, w, 3]: a sum of low-frequency cosines (small neighbouring-pixel steps keep the letterbox's ambiguous set small)"""
    y, x = np.meshgrid(np.arange(h) / max(h, w), np.arange(w) / max(h, w), indexing="ij")
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx = rng.uniform(-cycles, cycles, 2)
            img[..., c] += np.cos(2 * np.pi * (fy * y + fx * x) + rng.uniform(0, 2 * np.pi))
    lo, hi = img.min((0, 1)), img.max((0, 1))
    return np.rint((img - lo) / np.maximum(hi - lo, 1e-9) * 255).astype(np.uint8)


def persons(rng, n, h, w, invisible=0.2):
    """n random persons [n, 17, 3] spread over an h x w image (v = 2, or 0 with probability `invisible`)"""
    k = np.zeros((n, 17, 3), np.float32)
    for i in range(n):
        cx, cy = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h
        k[i, :, 0] = cx + rng.uniform(-0.25, 0.25, 17) * w
        k[i, :, 1] = cy + rng.uniform(-0.35, 0.35, 17) * h
        k[i, :, 2] = np.where(rng.uniform(size=17) < invisible, 0, 2)
    return k


def edge_persons(rng, h, w):
    """[n, 17, 3] fp32: the fit's edges -- nothing / two visible, collinear, v in {-1, 1, 2}, coordinates at +-1e5, a duplicate, off-frame
    points, NaN / +-inf coordinates on visible and on invisible keypoints"""
    out = list(persons(rng, 4, h, w))
    k = out[0].copy(); k[:, 2] = 0; out.append(k)                                   # nothing visible
    k = out[1].copy(); k[2:, 2] = 0; out.append(k)                                  # two visible
    k = out[1].copy(); k[:, 0] = k[:, 1] = 50.0; k[:, 2] = 2; out.append(k)          # one place
    k = out[2].copy(); k[:, 1] = 3.0 * k[:, 0] + 7.0; k[:, 2] = 2; out.append(k)     # collinear
    k = out[2].copy(); k[:, 2] = rng.choice(np.float32([-1, 1, 2]), 17); out.append(k)
    k = out[3].copy(); k[3, :2] = (1e5, -1e5); k[7, :2] = (-1e5, 1e5); out.append(k)
    out.append(out[0].copy())                                                         # a duplicated person
    k = out[1].copy(); k[:, 0] += 2.0 * w; out.append(k)                              # off-frame
    k = out[2].copy(); k[0, 2] = 2; k[0, 0] = np.nan; out.append(k)                   # NaN on the first (visible) keypoint
    k = out[3].copy(); k[2:5, 2] = 2; k[2, 1] = np.inf; k[4, 0] = -np.inf; out.append(k)
    k = out[0].copy(); k[:3, 2] = 0; k[0, 0] = np.nan; k[1, 1] = np.inf; out.append(k)   # non-finite but invisible
    k = out[1].copy(); k[:15, 2] = 0; k[15, 0] = np.nan; k[15, 2] = 2; k[16, 2] = 2; out.append(k)   # the fallback box over NaN + one point
    return np.stack(out).astype(np.float32)


def random_templates(rng, T, zero_weight=0.2):
    """[T, 17, 3] fp32 templates in the align frame, some joints of weight 0; template T - 1 duplicates template 0 when T > 2"""
    tp = np.zeros((T, 17, 3), np.float32)
    tp[..., :2] = rng.uniform(6, 58, (T, 17, 2))
    tp[..., 2] = np.where(rng.uniform(size=(T, 17)) < zero_weight, 0.0, rng.uniform(0.25, 2.0, (T, 17)))
    if T > 2:
        tp[T - 1] = tp[0]
    return tp


def posed_persons(rng, n, h, w, templates, invisible=0.15):
    """n persons [n, 17, 3] that look like people: a random template under a random similarity (30-80 % of the image's height, a small
    rotation) plus a few pixels of noise, so the fit fills the align frame with the person"""
    k = np.zeros((n, 17, 3), np.float32)
    for i in range(n):
        t = np.asarray(templates[rng.integers(len(templates))], np.float64)
        s = rng.uniform(0.3, 0.8) * h / S_ALIGN
        a = rng.uniform(-0.3, 0.3)
        R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        c = np.array([rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h])
        k[i, :, :2] = (t[:, :2] - S_ALIGN / 2) @ R.T + c + rng.normal(0, 0.02 * s * S_ALIGN, (17, 2))
        k[i, :, 2] = np.where(rng.uniform(size=17) < invisible, 0, 2)
    return k
