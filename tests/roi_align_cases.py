"""RoIAlign and the LevelMapper stated a second time, and the inputs that pin their discrete decisions (tests only; imports neither `oracle` nor `isegmi`).

References
  roi_align_f64          plain numpy from the operator's definition.  The RoI geometry (scaled corners, size clamp, bin size, sample coordinates) is computed step
                         by step in np.float32 -- every step one correctly rounded IEEE operation, in the order the kernels and the oracle use, so the sample
                         coordinates are the SAME numbers as theirs (the build has -ffp-contract=off) -- and everything after it (validity, clamps, taps, weights,
                         sum, mean) in float64.  count = max(gh * gw, 1).  Also returns S = sum |w| |v| per output element for rounding_bound().
  roi_align_grid_sample  the same operator through torch.nn.functional.grid_sample(bilinear, border, align_corners=True) in float64, times the validity mask
                         -1 <= v <= size, averaged per bin.  grid_sample renormalises the coordinates, so it is never bit-exact: tolerance tests only.
  level_f64              floor(4 + log2(sqrt(area) / 224 + 1e-6)) in float64, clamped to [k_min, k_max]; also returns the unfloored value (for LEVEL_BAND).
  rounding_bound         (gh gw + 9) 2^-24 S / (gh gw): the first-order rounding bound of the fp32 chain on identical sample coordinates.  Per sample: a weight
                         is a product of two factors of which each is exact or rounded once (l = v - floor(v) is exact, h = 1 - l rounds only when l < 1/2), so
                         <= 3 roundings; one more for weight * value; <= 3 for the sample's three adds: <= 7 per tap.  Then gh gw adds of the samples and one
                         division: gh gw + 1.  Total gh gw + 8 <= gh gw + 9 half-ulps-of-relative-error 2^-24 on terms whose magnitudes sum to S.

A `Case` is geometry only -- pyramid shapes, scales, k_min, rois [N, K, 4], counts [N], PH, aligned -- plus `tags` that say where a named RoI's first or last
sample must sit; features come from `make_feats(case, C)` so that one geometry runs through kernels that want different channel counts.  Feature kinds:
  "int"     integers in [-8, 8]: with power-of-two scales and bins every weight, product and sum is exact in fp32 and in fp16 (asserted on the CPU)
  "edge8"   integers in [-2, 2], but magnitude 8 (sign by channel) on the outermost rows and columns of every map: a sample that drops out changes the bin by
            >= 8 / 4 while the rounding bound stays near 1e-6
  "level"   the constant (level index + 1) on every map: the output names the level a kernel without an out_level argument chose
  "normal"  standard normal, rounded through fp16 so that the fp16 kernels see the same numbers"""
import numpy as np

F32, F64 = np.float32, np.float64
PYRAMID_SCALES = [0.25, 0.125, 0.0625, 0.03125]
PYR_A = [(56, 112), (28, 56), (14, 28), (7, 14)]   # a 224 x 448 image: the whole image is a level-4 RoI with bins of 2 x 4 (7 x 7) or 1 x 2 (14 x 14)
PYR_B = [(8, 8), (4, 4), (2, 2), (1, 1)]           # coarsest map 1 x 1: yl >= H - 1 at H == 1 takes both taps from row 0 (and column 0)
PYR_C = [(8, 32), (4, 16), (2, 8), (1, 4)]         # coarsest map 1 x W
PYR_D = [(48, 64), (24, 32), (12, 16), (6, 8)]     # the random / launch-shape families (a 192 x 256 image)
LEVEL_BAND = 4 * 2.0 ** -21   # 4 fp32 ulps of 4.0 (1.9e-6): `4.0f + t` rounds, and t carries the rounding of the area, sqrt, quotient, + 1e-6f and log2


# ----------------------------------------------------------------------------------------------------------------------------- references
def roi_geometry(roi, scale, PH, PW, g, aligned):
    """fp32, one IEEE operation at a time -> (ys [PH, gh], xs [PW, gw], gh, gw, rh, rw); g <= 0: the adaptive grid ceil(bin size)"""
    x1, y1, x2, y2 = (F32(v) for v in roi)
    sc, off = F32(scale), F32(0.5 if aligned else 0.0)
    sw, sh, ew, eh = x1 * sc - off, y1 * sc - off, x2 * sc - off, y2 * sc - off
    rw, rh = ew - sw, eh - sh
    if not aligned:
        rw = rw if rw > F32(1) else F32(1)
        rh = rh if rh > F32(1) else F32(1)
    bh, bw = rh / F32(PH), rw / F32(PW)
    gh = g if g > 0 else int(np.ceil(bh))
    gw = g if g > 0 else int(np.ceil(bw))

    def axis(start, b, P, n):
        n = max(n, 0)
        p = np.arange(P, dtype=F32)[:, None]
        i = np.arange(n, dtype=F32)[None, :]
        return ((start + p * b) + ((i + F32(0.5)) * b) / F32(max(n, 1))).astype(F32)

    return axis(sh, bh, PH, gh), axis(sw, bw, PW, gw), gh, gw, rh, rw


def axis_taps(v, size, variant=None):
    """float64: sample coordinates v -> (valid, lo, hi, weight of lo, weight of hi).  variant = a naive reading of one decision:
    "lo_closed" v <= -1 is outside; "hi_closed" v >= size is outside; "no_clamp" no clamp at 0 or size - 1 (taps outside the map read 0)"""
    v = np.asarray(v, F64)
    below = v <= -1 if variant == "lo_closed" else v < -1
    above = v >= size if variant == "hi_closed" else v > size
    valid = ~(below | above)
    if variant == "no_clamp":
        lo = np.floor(v).astype(np.int64)
        l = v - lo
        return valid, lo, lo + 1, 1.0 - l, l
    c = np.where(valid & (v > 0), v, 0.0)
    lo = c.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    c = np.where(top, lo.astype(F64), c)
    l = c - lo
    return valid, lo, hi, 1.0 - l, l


def _bin_matrix(v, size, variant):
    """[P, n] sample coordinates of one axis -> A [P, size]: A[p, i] = the total weight bin p puts on row (column) i"""
    P = v.shape[0]
    valid, lo, hi, wl, wh = axis_taps(v, size, variant)
    A = np.zeros((P, size + 2), F64)   # one guard element on each side for the no_clamp variant
    rows = np.broadcast_to(np.arange(P)[:, None], v.shape)
    ok = valid & (lo >= -1) & (hi <= size)
    np.add.at(A, (rows[ok], lo[ok] + 1), wl[ok])
    np.add.at(A, (rows[ok], hi[ok] + 1), wh[ok])
    return A[:, 1:size + 1]


def roi_align_f64(feat, roi, scale, PH, PW, g, aligned, variant=None):
    """feat [H, W, C], roi (x1, y1, x2, y2) in image coordinates -> (out [PH, PW, C] float64, S [PH, PW, C] = sum |w| |v|, (gh, gw)).
    A sample is valid iff its y AND its x are, and its four weights are products of a y and an x weight, so the double sum over the samples and their taps
    factors into Ay [PH, H] (weight of map row h in bin row ph) and Ax [PW, W]."""
    H, W = feat.shape[:2]
    ys, xs, gh, gw, _, _ = roi_geometry(roi, scale, PH, PW, g, aligned)
    Ay, Ax = _bin_matrix(ys, H, variant), _bin_matrix(xs, W, variant)
    f = np.asarray(feat, F64)
    count = max(gh * gw, 1)
    def pool(ay, ax, v):   # sum_h sum_w ay[p, h] ax[q, w] v[h, w, c]
        return np.tensordot(ax, np.tensordot(ay, v, (1, 0)), (1, 1)).transpose(1, 0, 2)

    return pool(Ay, Ax, f) / count, pool(np.abs(Ay), np.abs(Ax), np.abs(f)), (gh, gw)


def rounding_bound(S, gh, gw):
    n = max(gh * gw, 1)
    return (n + 9) * 2.0 ** -24 * S / n


def f16_bound(bound, ref):
    return bound + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25


def roi_align_grid_sample(feat, roi, scale, PH, PW, g, aligned):
    """torch.grid_sample form: border padding is the clamp to [0, size - 1], the validity mask is applied outside it"""
    import torch
    import torch.nn.functional as Fn
    H, W, Cc = feat.shape
    ys, xs, gh, gw, _, _ = roi_geometry(roi, scale, PH, PW, g, aligned)
    if gh <= 0 or gw <= 0:
        return np.zeros((PH, PW, Cc), F64)
    y, x = torch.from_numpy(ys.astype(F64).reshape(-1)), torch.from_numpy(xs.astype(F64).reshape(-1))
    ny = 2 * y / (H - 1) - 1 if H > 1 else torch.zeros_like(y)
    nx = 2 * x / (W - 1) - 1 if W > 1 else torch.zeros_like(x)
    grid = torch.stack(torch.broadcast_tensors(nx[None, :], ny[:, None]), -1)[None]          # [1, PH gh, PW gw, (x, y)]
    img = torch.from_numpy(np.asarray(feat, F64)).permute(2, 0, 1)[None]
    smp = Fn.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]   # [C, PH gh, PW gw]
    mask = (((y >= -1) & (y <= H))[:, None] & ((x >= -1) & (x <= W))[None, :]).to(smp.dtype)
    smp = (smp * mask).reshape(Cc, PH, gh, PW, gw)
    return smp.mean(dim=(2, 4)).permute(1, 2, 0).numpy()


def level_f64(boxes, k_min=2, k_max=5):
    """boxes [n, 4] -> (level [n] int, t [n] = 4 + log2(sqrt(area) / 224 + 1e-6) in float64 on the fp32 corners)"""
    b = np.asarray(boxes, F32).astype(F64).reshape(-1, 4)
    area = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
    with np.errstate(invalid="ignore"):
        t = 4.0 + np.log2(np.sqrt(area) / 224.0 + 1e-6)
    # a negative area (one side reversed by more than a pixel) has no level: k_min, which is also all a single-level mapper can say
    return np.clip(np.floor(np.where(np.isnan(t), k_min, t)), k_min, k_max).astype(np.int64), t


def in_level_band(t):
    return np.abs(t - np.round(t)) < LEVEL_BAND


# ----------------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, shapes, scales, rois, PH, aligned, kind, k_min=2, counts=None, N=2, tags=(), exact=False, seed=0):
        rois = np.asarray(rois, F32).reshape(-1, 4)
        if counts is None:   # spread the list over N images
            K = -(-len(rois) // N)
            counts = [min(K, max(len(rois) - n * K, 0)) for n in range(N)]
            full = np.zeros((N * K, 4), F32)
            full[:len(rois)] = rois
            rois = full
        self.name, self.shapes, self.scales, self.k_min = name, list(shapes), list(scales), k_min
        self.counts = np.asarray(counts, np.int32)
        self.N = len(self.counts)
        self.K = len(rois) // self.N
        self.rois = rois.reshape(self.N, self.K, 4)
        self.PH = self.PW = PH
        self.aligned, self.kind, self.exact, self.seed = aligned, kind, exact, seed
        self.tags = list(tags)   # (flat row, axis "y" | "x", "first" | "last", coordinate or None, valid, label)
        self.exact_rows = None   # with exact False: the flat rows (n * K + k) that are exact all the same

    @property
    def k_max(self):
        return self.k_min + len(self.shapes) - 1

    def exact_mask(self):
        """[N, K] bool: the rows whose answer is exact in fp32 by construction"""
        m = np.zeros(self.N * self.K, bool)
        if self.exact:
            m[:] = True
        elif self.exact_rows is not None:
            m[list(self.exact_rows)] = True
        m = m.reshape(self.N, self.K)
        for n in range(self.N):
            m[n, int(self.counts[n]):] = False
        return m

    def rows(self):
        """(n, k) of every RoI inside its image's count"""
        return [(n, k) for n in range(self.N) for k in range(int(self.counts[n]))]


def make_feats(case, Cc):
    """-> one [N, H, W, C] float32 map per level, every value representable in fp16"""
    rng = np.random.default_rng(1000 + case.seed)
    out = []
    for li, (h, w) in enumerate(case.shapes):
        shape = (case.N, h, w, Cc)
        if case.kind == "int":
            f = rng.integers(-8, 9, shape).astype(F32)
        elif case.kind == "edge8":
            f = rng.integers(-2, 3, shape).astype(F32)
            rim = np.where(np.arange(Cc) % 2 == 0, 8.0, -8.0).astype(F32)
            f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = rim, rim, rim, rim
        elif case.kind == "level":
            f = np.full(shape, li + 1, F32)
        else:
            f = rng.standard_normal(shape).astype(np.float16).astype(F32)
        out.append(f)
    return out


def reference(case, feats, levels, g, variant=None):
    """-> (ref [N, K, PH, PW, C] float64, S, grids [N, K, 2]); rows past counts are zero.  levels [N, K]: the level of every RoI"""
    Cc = feats[0].shape[3]
    ref = np.zeros((case.N, case.K, case.PH, case.PW, Cc), F64)
    S = np.zeros_like(ref)
    grids = np.ones((case.N, case.K, 2), np.int64)
    for n, k in case.rows():
        li = int(levels[n, k]) - case.k_min
        ref[n, k], S[n, k], grids[n, k] = roi_align_f64(feats[li][n], case.rois[n, k], case.scales[li], case.PH, case.PW, g, case.aligned, variant)
    return ref, S, grids


def run_oracle(ora, case, feats, g):
    """the CPU oracle (passed in: this module does not import it) -> (out [N, K, PH, PW, C] float32 with zero rows past counts, levels [N, K])"""
    out = np.zeros((case.N, case.K, case.PH, case.PW, feats[0].shape[3]), F32)
    levels = np.full((case.N, case.K), case.k_min, np.int64)
    for n in range(case.N):
        c = int(case.counts[n])
        if c == 0:
            continue
        lv = ora.level_map(case.rois[n, :c], case.k_min, case.k_max)
        levels[n, :c] = lv
        for L in np.unique(lv):
            idx = np.nonzero(lv == L)[0]
            r5 = np.concatenate([np.full((len(idx), 1), n, F32), case.rois[n, idx]], 1)
            out[n, idx] = ora.roi_align(feats[L - case.k_min], r5, case.scales[L - case.k_min], case.PH, case.PW, g, case.aligned)
    return out, levels


def bound_of(S, grids):
    n = np.maximum(grids[..., 0] * grids[..., 1], 1).astype(F64)[:, :, None, None, None]
    return (n + 9) * 2.0 ** -24 * S / n


def _span(first, b, P, scale, aligned):
    """image-coordinate (lo, hi) of a RoI side whose bins are b map pixels and whose first sample (grid 2) sits at `first`"""
    s = first - b / 4 + (0.5 if aligned else 0.0)
    return s / scale, (s + P * b) / scale


def _ulps(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def _edge_rois(H, W, scale, P, aligned, b, mid_y, mid_x):
    """The five placements of a first / last sample on y (x mid-map) and on x (y mid-map) -> (rois, tags).  mid_*: first-sample coordinate of the other axis"""
    rois, tags = [], []
    last = (P - 1) * b + b / 2   # last sample - first sample
    for axis, size in (("y", H), ("x", W)):
        for which, coord, label in (("first", -1.0, "at -1: valid, clamps to 0"), ("first", 0.0, "at 0"), ("last", size - 1.0, "at size - 1"),
                                    ("last", size - 0.5, "between size - 1 and size"), ("last", float(size), "at size: valid, both taps size - 1")):
            lo, hi = _span(coord if which == "first" else coord - last, b, P, scale, aligned)
            mlo, mhi = _span(mid_x if axis == "y" else mid_y, b, P, scale, aligned)
            tags.append((len(rois), axis, which, coord, True, label))
            rois.append([mlo, lo, mhi, hi] if axis == "y" else [lo, mlo, hi, mhi])
    return rois, tags


def exact_cases(PH, aligned):
    """Integer features, power-of-two scales and bins: fp32 (and fp16) arithmetic is exact, so a kernel must return the float64 value bit for bit whatever
    its summation order.  One Case per pyramid."""
    cases = []
    # ---- pyramid A: level 2 (small RoIs, bins of 1 map pixel) carries the edges; levels 3..5 carry 14-pixel RoIs (bins of 2 or 1)
    (H, W), s = PYR_A[0], 0.25
    rois, tags = _edge_rois(H, W, s, PH, aligned, 1.0, 10.5, 20.5)
    for axis, size in (("y", H), ("x", W)):   # wholly outside on each of the four sides
        for which, first in (("last", -PH - 2.25), ("first", size + 1.25)):
            lo, hi = _span(first, 1.0, PH, s, aligned)
            mlo, mhi = _span(12.5, 1.0, PH, s, aligned)
            tags.append((len(rois), axis, which, None, False, "wholly outside"))
            rois.append([mlo, lo, mhi, hi] if axis == "y" else [lo, mlo, hi, mhi])
    rois.append([0, 0, 448, 224])                                # the whole level-4 map
    rois.append([8, 16, 8 + 2 * PH, 16 + 2 * PH])                # bins of half a map pixel at level 2
    rois += [[16, 8, 128, 120], [32, 16, 256, 240], [0, -64, 448, 384], [200, 100, 648, 548]]   # 14 map pixels at levels 3, 4, 5, 5 (the last two hang outside)
    if aligned:   # defined values under a fixed grid (all of a bin's samples coincide along the flat axis); the zero-grid case under the adaptive one
        rois += [[40, 24, 40, 24 + 4 * PH], [40, 24, 40 + 4 * PH, 24], [40 + 4 * PH, 24 + 4 * PH, 40, 24], [40, 24, 40, 24]]
    cases.append(Case("exact_A", PYR_A, PYRAMID_SCALES, rois, PH, aligned, "int", tags=tags, exact=True, seed=1))
    # ---- pyramids B (1 x 1) and C (1 x W): level-5 RoIs (14 coarse pixels) whose first samples land on -1, (-1, 0), 0, (0, 1) and 1 == size of the 1-pixel axis
    b = 14.0 / PH
    for name, pyr in (("exact_B", PYR_B), ("exact_C", PYR_C)):
        H5, W5 = pyr[3]
        rois, tags = [], []
        for axis, size in (("y", H5), ("x", W5)):
            for coord, valid in ((-1.0, True), (0.0, True), (float(size), True), (size - b, True), (-1.0 - b / 2, False)):
                lo, hi = _span(coord, b, PH, 1 / 32, aligned)
                mlo, mhi = _span(-0.5, b, PH, 1 / 32, aligned)
                tags.append((len(rois), axis, "first", coord, valid and coord >= -1, "first sample on a map of size %d" % size))
                rois.append([mlo, lo, mhi, hi] if axis == "y" else [lo, mlo, hi, mhi])
        rois += [[0, 0, 4 * PH, 4 * PH], [-4, -8, 108, 104], [16, 0, 240, 224]]   # levels 2, 3, 4 of the small pyramid
        cases.append(Case(name, pyr, PYRAMID_SCALES, rois, PH, aligned, "int", tags=tags, exact=True, seed=2 if name == "exact_B" else 3))
    return cases


def ulp_neighbour_case(PH, aligned):
    """The -1 and `size` placements of exact_cases moved by fp32 ulps until the first sample is below -1 / the last above size in the fp32 geometry (the tag
    says so and the CPU test asserts it).  The near edge moves y1 (x1) down.  The far edge moves y2 (x2) up: moving y1 up shrinks the bins and leaves the last
    sample within 0.04 ulp of where it was.  The rim of every map holds magnitude 8 (kind "edge8"), so the sample that left is >= 2^20 rounding bounds."""
    (H, W), s = PYR_A[0], 0.25
    base, btags = _edge_rois(H, W, s, PH, aligned, 1.0, 10.5, 20.5)
    rois, tags = [], []
    for (row, axis, which, coord, _, _) in btags:
        if coord not in (-1.0, float(H if axis == "y" else W)) or (which == "first") != (coord == -1.0):
            continue
        size = H if axis == "y" else W
        idx = (1 if axis == "y" else 0) + (0 if which == "first" else 2)
        for k in range(1, 9):
            r = np.array(base[row], F32)
            r[idx] = _ulps(r[idx], -k if which == "first" else k)
            ys, xs, *_ = roi_geometry(r, s, PH, PH, 2, aligned)
            v = (ys if axis == "y" else xs)
            if (which == "first" and v[0, 0] < -1) or (which == "last" and v[-1, -1] > size):
                break
        tags.append((len(rois), axis, which, None, False, "%d ulp(s) beyond %s" % (k, "-1" if which == "first" else "size")))
        rois.append(r)
        tags.append((len(rois), axis, which, coord, True, "the exact neighbour"))
        rois.append(base[row])
    return Case("ulp_neighbours", PYR_A, PYRAMID_SCALES, rois, PH, aligned, "edge8", tags=tags, seed=4)


def small_roi_case(PH, aligned):
    """RoIs smaller than one map pixel (aligned 0: clamped to 1 x 1; aligned 1: not clamped), a RoI of exactly one pixel (`> 1` does not fire: same value), one
    an ulp above it, and bins that are no power of two.  Not exact: compared under rounding_bound."""
    rois = [[40, 40, 41, 42], [40.5, 41.25, 40.75, 41.5], [40, 40, 44, 44], [40, 40, _ulps(44, 1), _ulps(44, 1)], [40, 40, 43.5, 43.5],
            [3.3, 7.7, 61.2, 45.1], [-9.5, -7.25, 30.1, 50.9], [400, 180, 470, 250], [101.3, 17.9, 333.3, 202.2], [0, 0, 447, 223], [5, 5, 440, 215]]
    return Case("small_and_odd", PYR_A, PYRAMID_SCALES, rois, PH, aligned, "normal", seed=5)


LEVEL_SIDES = [112, 224, 448]


def level_boxes(side):
    """[0, 0, side - 1 + d, side - 1], 164 boxes: d on a 1 / 1024 grid of +-80 steps around the float64 flip (sqrt(area) / 224 + 1e-6 = side / 224 at
    d* = -2 * 224e-6, about -29 to -117 fp32 ulps of side - 1), plus the 2 fp32 neighbours of x2 on either side of the flip.  The neighbours always lie in
    LEVEL_BAND (one ulp of x2 moves the unfloored level by 5e-8); the grid keeps the band's share below 5 %."""
    flip = (side - 224e-6) ** 2 / side - side
    x2 = [F32(side - 1 + round(flip * 1024) / 1024 + j / 1024) for j in range(-80, 80)]
    upper = lambda v: level_f64([[0, 0, v, side - 1]])[1][0] >= round(np.log2(side / 224.0)) + 4
    c = F32(side - 1 + flip)
    while upper(c):
        c = _ulps(c, -1)
    while not upper(c):
        c = _ulps(c, 1)       # the first fp32 x2 of the upper level
    x2 += [_ulps(c, j) for j in range(-2, 2)]
    return np.array([[0, 0, v, side - 1] for v in x2], F32)


def level_case(PH):
    """Three images, one boundary each (112 / 224 / 448), on 32 x 32 maps that hold (level index + 1): every sample is inside, every output element of a RoI
    is its level's constant up to the weights' rounding.  Plus areas far below level 2 and far above level 5."""
    per = [np.concatenate([level_boxes(s), np.array([[3, 3, 5, 4], [10, 10, 10, 10], [0, 0, 900, 900], [0, 0, 30000, 20000]], F32)]) for s in LEVEL_SIDES]
    K = len(per[0])
    return Case("levels", [(32, 32)] * 4, PYRAMID_SCALES, np.concatenate(per), PH, 0, "level", counts=[K, K, K], seed=6)


def single_level_case(PH):
    """k_min 4 with a single level: every box, whatever its area, maps to level 4"""
    rois = np.concatenate([level_boxes(448)[::40], np.array([[3, 3, 5, 4], [0, 0, 900, 900], [64, 32, 64 + 16 * PH, 32 + 16 * PH]], F32)])
    return Case("single_level", [(24, 40)], [1 / 16], rois, PH, 0, "int", k_min=4, seed=7)


def adaptive_case(PH, aligned):
    """sampling = 0 on one stride-16 map (the C4 pooler: k_min 4, one level).  tags: (row, "g", None, (gh, gw), True, label)"""
    s, o = 16.0, (8.0 if aligned else 0.0)   # o: image offset that puts the scaled corner on an integer under aligned
    y0, x0 = 32 + o, 48 + o
    rois, tags = [], []

    def add(r, grid, label):
        tags.append((len(rois), "g", None, grid, True, label))
        rois.append(r)

    add([x0, y0, x0 + 2 * PH * s, y0 + 2 * PH * s], (2, 2), "bin size exactly 2")
    for k in range(1, 9):
        up = _ulps(y0 + 2 * PH * s, k)
        if roi_geometry([x0, y0, x0 + 2 * PH * s, up], 1 / 16, PH, PH, 0, aligned)[2] == 3:
            break
    add([x0, y0, x0 + 2 * PH * s, up], (3, 2), "bin height %d ulp(s) above 2" % k)
    add([x0, y0, x0 + PH * s, y0 + PH * s], (1, 1), "bin size 1")
    add([x0, y0, x0 + PH * s / 2, y0 + PH * s / 2], (1, 1), "bin size 1/2")
    add([x0, y0 - 16, x0 + PH * s, y0 - 16 + 4 * PH * s], (4, 1), "tall and thin")
    add([x0, y0, x0 + 4 * PH * s, y0 + PH * s], (1, 4), "wide and flat")
    add([-40, 500, 1000, 700], None, "hangs over three sides")
    add([x0, y0, x0, y0 + PH * s], (1, 0) if aligned else (1, 1), "zero width")
    add([x0, y0, x0 + PH * s, y0], (0, 1) if aligned else (1, 1), "zero height")
    add([x0 + PH * s, y0 + PH * s, x0, y0], (-1, -1) if aligned else (1, 1), "reversed")
    add([x0 + PH * s, y0, x0, y0 + PH * s], (1, -1) if aligned else (1, 1), "reversed in x")
    add([x0, y0, x0, y0], (0, 0) if aligned else (1, 1), "a point")
    case = Case("adaptive", [(40, 56)], [1 / 16], rois, PH, aligned, "int", k_min=4, tags=tags, seed=8, N=1)
    case.exact_rows = [0, 2, 3, 4, 5] + ([7, 8, 9, 10, 11] if aligned else [])   # power-of-two bins, and the empty grids (+0)
    return case


def random_boxes(rng, n, W, H, lo=6.0, hi=400.0):
    c = rng.uniform(0, 1, (n, 2)) * [W, H]
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)   # not clipped: some hang outside


def launch_case(N, K, counts, PH, seed=0):
    """Random boxes over PYR_D for the launch-shape tests (the caller chooses C)"""
    rng = np.random.default_rng(77 + seed)
    return Case("launch_N%d_K%d" % (N, K), PYR_D, PYRAMID_SCALES, random_boxes(rng, N * K, 256, 192), PH, 0, "normal", counts=counts, seed=9 + seed)
