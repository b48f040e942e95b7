"""Inputs of the decode kernel's edge tests (TEST INFRASTRUCTURE ONLY; tests/test_keypoint_fp64_cpu.py, tests/test_keypoint_edges_gpu.py): the exact-input
cases held against fp64 (tests/keypoint_fp64.py), the thread-layout sweep, the non-finite maps and the operator's limits, each built once per process with
its restated results (tests/keypoint_ref.py) and never modified."""
import functools

import numpy as np

import keypoint_fp64 as k64
import keypoint_ref as kr

F = np.float32
S, K = 56, 17
THREADS = 256


def layout(wc, hc):
    """The kernel's work split, from its definition: -> (ncol, nseg, rows_per)"""
    ncol = min(wc, THREADS)
    nseg = THREADS // ncol
    return ncol, nseg, -(-hc // nseg)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _box(i, wc, hc, cut=(0.5, 0.75, 0.25, 0.0)):
    """A box with a non-zero, non-integer origin whose sides ceil to (wc, hc); sides are multiples of 1/4, so x2 - x1 is exact in fp32.  Sides of 1 stay 1
    (w < 1 would also give 1)."""
    x1, y1 = 3.25 + 1.5 * (i % 7), 2.75 + 2.5 * (i % 5)
    w, h = wc - cut[i % 4], hc - cut[(i // 4 + 1) % 4]
    return (x1, y1, x1 + w, y1 + h)


# ---- exact inputs (issue item 2): every product and sum of the fp32 chain is exact, so the kernel must equal fp64 bit for bit
EXACT_SIDES = (7, 14, 28, 56, 112)
EXACT_CASES = tuple((hc, wc, 100, False) for hc in EXACT_SIDES for wc in EXACT_SIDES) + ((448, 56, 100, False), (56, 448, 100, False),
                                                                                           (224, 224, 2, True), (224, 56, 2, True))


def _integers(rng, amp, k):
    """[S, S, k] integers in -amp .. amp - 1 with one pixel per channel raised to amp (at the identity size a map's own maximum would repeat otherwise)"""
    m = rng.integers(-amp, amp, (S, S, k)).astype(F)
    p = rng.integers(0, S * S, k)
    m.reshape(S * S, k)[p, np.arange(k)] = amp
    return m


def _tiled(rng, amp, k):
    """[S, S, k]: a 14 x 14 tile of integers in -amp .. amp repeated 4 x 4 -- the resized values repeat with it exactly, so away from the clamped border the
    maximum is held by several positions in different rows, columns, waves and segments"""
    return np.ascontiguousarray(np.tile(rng.integers(-amp, amp + 1, (14, 14, k)), (4, 4, 1)).astype(F))


@functools.lru_cache(maxsize=None)
def exact_batch():
    """-> (heat [32, S, S, K], boxes [1, 32, 4], count [1], cases, want_kpt [n, K, 3] fp32, want_score [n, K] fp64, n_max [n, K]) from the fp64 reference.
    Integer maps of |m| <= 100 (all 17 channels different; a channel whose fp64 maximum is not unique is drawn again) and, in the two tie cases, of
    |m| <= 2, whose maxima repeat many times: there "the lower row-major position wins" is held against fp64."""
    rng = np.random.default_rng(2)
    n, cap = len(EXACT_CASES), 32
    heat = np.full((cap, S, S, K), np.nan, F)
    boxes = np.full((1, cap, 4), np.nan, F)
    kpt, score, nmax = np.zeros((n, K, 3), F), np.zeros((n, K), np.float64), np.zeros((n, K), np.int64)
    for i, (hc, wc, amp, ties) in enumerate(EXACT_CASES):
        boxes[0, i] = _box(i, wc, hc)
        assert k64.sides(boxes[0, i])[2:] == (wc, hc)
        maps = _tiled(rng, amp, K) if ties else _integers(rng, amp, K)
        kpt[i], score[i], _, nmax[i] = k64.decode_one(maps, boxes[0, i])
        for _ in range(20):
            again = np.nonzero(nmax[i] > 1)[0]
            if ties or not len(again):
                break
            maps[:, :, again] = _integers(rng, amp, len(again))
            kpt[i], score[i], _, nmax[i] = k64.decode_one(maps, boxes[0, i])
        heat[i] = maps
    count = np.array([n], np.int32)
    return _freeze(heat, boxes, count) + (EXACT_CASES,) + _freeze(kpt, score, nmax)


# ---- the thread-layout sweep (items 5 and 3)
SWEEP_WC = (1, 2, 3, 63, 64, 65, 85, 86, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1023)
SWEEP_HC = (1, 2, 3, 4, 5, 57, 200)
SWEEP_CAP = 20                       # one image per hc, its 19 widths in slots 0..18: count < cap in every image
PLACES = ("top-left", "top-right", "bottom-left", "bottom-right", "top-mid", "bottom-mid", "left-mid", "right-mid", "segment-first-row", "segment-last-row",
          "second-stride")            # channels 0..10; channels 11..16 hold smooth-peak maps at random centres


def middle_segment(wc, hc):
    """-> (first row, last row) of the middle segment that has rows (segment nseg // 2, or the last one that is not empty)"""
    _, nseg, rows_per = layout(wc, hc)
    seg = min(nseg // 2, (hc - 1) // rows_per)
    return seg * rows_per, min(seg * rows_per + rows_per, hc) - 1


def place_target(k, wc, hc):
    """The output position (y, x) channel k < 11 aims at"""
    ya, yb = middle_segment(wc, hc)
    return ((0, 0), (0, wc - 1), (hc - 1, 0), (hc - 1, wc - 1), (0, wc // 2), (hc - 1, wc // 2), (hc // 2, 0), (hc // 2, wc - 1),
            (ya, wc // 3), (yb, (2 * wc) // 3), (hc // 3, 256 if wc > 256 else wc // 2))[k]


def _peak(rng, cy, cx, sigma, noise):
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    return 8.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma ** 2)) + noise * rng.standard_normal((S, S))


def sweep_maps(seed, wc, hc):
    """[S, S, K]: channels 0..10 a sharp peak (sigma 1.5, noise 0.002) centred where the target position samples the source; channels 11..16 the smooth-peak
    maps of tests/keypoint_cases.py (sigma 3, noise 0.05) at random centres"""
    rng = np.random.default_rng(seed)
    m = np.empty((S, S, K), F)
    for k in range(K):
        if k < len(PLACES):
            ty, tx = place_target(k, wc, hc)
            m[:, :, k] = _peak(rng, (ty + 0.5) * S / hc - 0.5, (tx + 0.5) * S / wc - 0.5, 1.5, 0.002)
        else:
            cy, cx = rng.uniform(0, S - 1, 2)
            m[:, :, k] = _peak(rng, cy, cx, 3.0, 0.05)
    return m


@functools.lru_cache(maxsize=None)
def sweep_batch():
    """-> (heat [7 * 20, S, S, K], boxes [7, 20, 4], count [7], want_kpt, want_kscore, pos {(n, c): [K]}) -- 133 detections, restated"""
    N, cap = len(SWEEP_HC), SWEEP_CAP
    heat = np.full((N * cap, S, S, K), np.nan, F)
    boxes = np.full((N, cap, 4), np.nan, F)
    count = np.full(N, len(SWEEP_WC), np.int32)
    kpt, ks, pos = np.zeros((N, cap, K, 3), F), np.zeros((N, cap, K), F), {}
    for n, hc in enumerate(SWEEP_HC):
        for c, wc in enumerate(SWEEP_WC):
            boxes[n, c] = _box(n * cap + c, wc, hc)
            assert kr.box_sizes(boxes[n, c])[2:] == (wc, hc)
            heat[n * cap + c] = sweep_maps(1000 * n + c, wc, hc)
            kpt[n, c], ks[n, c], pos[(n, c)] = kr.decode_one(heat[n * cap + c], boxes[n, c])
    return _freeze(heat, boxes, count, kpt, ks) + (pos,)


def places_hit():
    """{place: [(hc, wc), ...]} -- the detections whose restated maximum of the place's channel lies exactly on the place"""
    pos = sweep_batch()[5]
    hit = {p: [] for p in PLACES}
    for n, hc in enumerate(SWEEP_HC):
        for c, wc in enumerate(SWEEP_WC):
            for k, name in enumerate(PLACES):
                ty, tx = place_target(k, wc, hc)
                if int(pos[(n, c)][k]) == ty * wc + tx:
                    hit[name].append((hc, wc))
    return hit


# ---- non-finite maps (item 4)
NAN_SIZES = ((112, 112), (300, 40))   # (hc, wc): 2 segments of 56 rows in 4 waves; 6 segments of 50 rows, 16 idle threads
NAN_KINDS = ("nan-mid", "nan-last-row", "all-nan", "inf-one", "all-neg-inf", "nan-one-channel")
NAN_CHANNEL = 7


def nan_maps(kind, seed):
    m = sweep_maps(seed, 112, 112)
    for k in range(K):
        if kind == "nan-mid":
            m[20 + k, 30 - k, k] = np.nan
        elif kind == "nan-last-row":
            m[S - 1, 5 + 2 * k, k] = np.nan
        elif kind == "all-nan":
            m[:, :, k] = np.nan
        elif kind == "inf-one":
            m[25 + k % 5, 20 + k, k] = np.inf
        elif kind == "all-neg-inf":
            m[:, :, k] = -np.inf
        elif kind == "nan-one-channel" and k == NAN_CHANNEL:
            m[27, 31, k] = np.nan
    return m


@functools.lru_cache(maxsize=None)
def nan_batch():
    """-> (heat [12, S, S, K], boxes [2, 6, 4], count [2], want_kpt, want_kscore, pos [2, 6, K]): image n holds the six kinds at NAN_SIZES[n]"""
    N, cap = len(NAN_SIZES), len(NAN_KINDS)
    heat, boxes = np.zeros((N * cap, S, S, K), F), np.zeros((N, cap, 4), F)
    pos = np.zeros((N, cap, K), np.int64)
    for n, (hc, wc) in enumerate(NAN_SIZES):
        for c, kind in enumerate(NAN_KINDS):
            heat[n * cap + c] = nan_maps(kind, 50 + c)
            boxes[n, c] = _box(n * cap + c, wc, hc)
    count = np.full(N, cap, np.int32)
    with np.errstate(invalid="ignore"):
        kpt, ks = kr.decode(heat, boxes, count)
        for n in range(N):
            for c in range(cap):
                pos[n, c] = kr.decode_one(heat[n * cap + c], boxes[n, c])[2]
    return _freeze(heat, boxes, count, kpt, ks, pos)


def same_floats(a, b):
    """Bit equality of the finite and infinite values and the same places NaN (a NaN's sign and payload are the producing machine's: x86 makes the
    default NaN negative, the GPU positive)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


# ---- the operator's limits (item 6)
LIMIT_SIDES = ((1, 1), (5, 3), (57, 129), (70, 300))   # (hc, wc)


@functools.lru_cache(maxsize=None)
def limit_batch(s, k):
    """Heat maps of side s with k keypoints, four boxes and an empty slot -> (heat, boxes [1, 5, 4], count, want_kpt, want_kscore)"""
    rng = np.random.default_rng(100 * s + k)
    cap = len(LIMIT_SIDES) + 1
    heat = rng.standard_normal((cap, s, s, k)).astype(F)
    heat[-1] = np.nan
    boxes = np.full((1, cap, 4), np.nan, F)
    for i, (hc, wc) in enumerate(LIMIT_SIDES):
        boxes[0, i] = _box(i, wc, hc)
    count = np.array([cap - 1], np.int32)
    return _freeze(heat, boxes, count, *kr.decode(heat, boxes, count))


GRID_N, GRID_CAP, GRID_DISTINCT = 255, 257, 251   # 255 * 257 = 65535 workgroup rows; slot r holds combination r % 251 (251 is prime to both)


@functools.lru_cache(maxsize=None)
def grid_batch():
    """N * cap = 65535 at S = 2, K = 1: 251 different (box, map) combinations with resized sides 1..3, restated once each and repeated over the slots; image
    n has count (37 n) % 258, so empty, partly filled and full images occur -> (heat, boxes, count, want_kpt, want_kscore)"""
    rng = np.random.default_rng(65535)
    D = GRID_DISTINCT
    dheat = rng.standard_normal((D, 2, 2, 1)).astype(F)
    dbox = np.array([_box(i, 1 + i % 3, 1 + (i // 3) % 3) for i in range(D)], F)
    dk, ds = kr.decode(dheat, dbox[None], np.array([D], np.int32))
    r = np.arange(GRID_N * GRID_CAP) % D
    heat, boxes = dheat[r], dbox[r].reshape(GRID_N, GRID_CAP, 4)
    count = ((37 * np.arange(GRID_N)) % (GRID_CAP + 1)).astype(np.int32)
    livemask = (np.arange(GRID_CAP)[None, :] < count[:, None])
    kpt = np.where(livemask[:, :, None, None], dk[0][r].reshape(GRID_N, GRID_CAP, 1, 3), F(0))
    ks = np.where(livemask[:, :, None], ds[0][r].reshape(GRID_N, GRID_CAP, 1), F(0))
    return _freeze(np.ascontiguousarray(heat), np.ascontiguousarray(boxes), count, kpt.astype(F), ks.astype(F))


LONG_BOXES = ((2.5, 1.25, 3.0, 16385.0),        # 16384 x 1 (hc x wc): 256 segments of 64 rows
              (1.25, 2.5, 16385.0, 3.25),       # 1 x 16384: 64 strides of 256 columns
              (0.5, 0.25, 20000.5, 2.0))        # w = 20000: the resized width is cut at 16384, cw = 20000 / 16384; hc = 2


@functools.lru_cache(maxsize=None)
def long_batch():
    from keypoint_cases import smooth_peak_maps
    cap = len(LONG_BOXES)
    heat = np.stack([smooth_peak_maps(70 + i) for i in range(cap)])
    boxes = np.array(LONG_BOXES, F)[None]
    count = np.array([cap], np.int32)
    return _freeze(heat, boxes, count, *kr.decode(heat, boxes, count))
