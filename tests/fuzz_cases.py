"""Case builders of the tail / encoder / painter property tests (tests/test_fuzz_cases_cpu.py, tests/test_fuzz_tails_gpu.py).  numpy only.

One builder per operator: build_<op>(profile, seed) -> dict, a pure function of its two arguments.  The dict holds everything the device call and the
reference need, plus `reached`: the set of named conditions the case holds, each decided by a predicate over the finished inputs (not by the profile
name).  A profile CONSTRUCTS its condition -- it copies a score onto the cut, plants a zero run, sizes a window so that it ends on a chunk border -- so
`profile in reached` for every seed; nothing is drawn and thrown away.  Values that decide something are quantised (multiples of 1/8) so that ties and
threshold hits are common; sizes are the smallest at which the kernel's own structure is crossed.

ref_<op>(case) -> the reference's answer as a dict of arrays (tests/*_ref.py, oracle/ora.py), the form the GPU test compares bit for bit.
OPS maps an operator's name to its builder, reference and profiles.
"""
import numpy as np

import cocoeval_ref
import keypoint_ref
import pose_handoff_ref
import render_ref
import resample_ref

F = np.float32


def bytes_of(x):
    """everything a run or a reference returned, as one bytes object (dicts in key order, lists in order, None as nothing)"""
    if x is None:
        return b""
    if isinstance(x, dict):
        return b"".join(bytes_of(x[k]) for k in sorted(x, key=str))
    if isinstance(x, (list, tuple)):
        return b"".join(bytes_of(v) for v in x)
    if isinstance(x, (bytes, str)):
        return x.encode() if isinstance(x, str) else x
    return np.ascontiguousarray(x).tobytes()


def _rng(op, profile, seed):
    return np.random.default_rng([sum(map(ord, op)), sum(map(ord, profile)) * 131 + len(profile), int(seed)])


# ============================================================================================================ RleSet / rle_iou on hand-written counts
RLE_COUNTS_PROFILES = ("zero_run_first", "zero_1run_inside", "zero_0run_inside", "zero_run_last", "only_zero_runs_then_full", "more_than_256_runs_with_zeros")
PREFIX_ROUND = 256      # coco_rle_prefix_kernel scans 256 runs per round and carries the sums into the next


def _canonical_counts(rng, P, runs, leading_one=False):
    """`runs` positive runs that add up to P (runs <= P), a zero in front when the mask starts set: what rleEncode would produce"""
    cuts = np.sort(rng.choice(np.arange(1, P), runs - 1, replace=False)) if runs > 1 else np.zeros(0, np.int64)
    c = np.diff(np.concatenate([[0], cuts, [P]])).astype(np.int64).tolist()
    return [0] + c if leading_one else c


def rle_conditions(counts):
    """The zero-run conditions a count list holds, by index parity (even index: 0-run, odd index: 1-run)"""
    c = list(counts)
    n = len(c)
    out = set()
    if n >= 2 and c[0] == 0 and c[1] == 0:
        out.add("zero_run_first")
    if any(c[i] == 0 for i in range(1, n - 1, 2)):
        out.add("zero_1run_inside")
    if any(c[i] == 0 and c[i - 1] > 0 and c[i + 1] > 0 for i in range(2, n - 1, 2)):
        out.add("zero_0run_inside")
    if n >= 2 and c[-1] == 0:
        out.add("zero_run_last")
    if n >= 2 and all(v == 0 for v in c[:-1]) and c[-1] > 0:
        out.add("only_zero_runs_then_full")
    if n > PREFIX_ROUND and any(c[i] == 0 for i in range(1, n, 2)) and any(c[i] == 0 for i in range(2, n, 2)):
        out.add("more_than_256_runs_with_zeros")
    return out


def _plant(rng, profile, P):
    """One count list over P pixels that holds the profile's condition"""
    if profile == "only_zero_runs_then_full":
        return [0] * int(rng.integers(2, 9)) + [P]          # an even number of zeros in front: the empty mask; an odd number: the full one
    if profile == "more_than_256_runs_with_zeros":
        c = _canonical_counts(rng, P, int(rng.integers(PREFIX_ROUND + 4, min(P, 2 * PREFIX_ROUND + 40) + 1)))
        for i in (PREFIX_ROUND - 1, PREFIX_ROUND, PREFIX_ROUND + 1):   # zeros of both parities on both sides of the scan's seam, and a few elsewhere
            c.insert(i, 0)
        for i in sorted(rng.integers(1, len(c), 4).tolist()):
            c.insert(i, 0)
        return c
    runs = int(rng.integers(3, min(P, 24) + 1))
    c = _canonical_counts(rng, P, runs, leading_one=bool(rng.integers(0, 2)) and profile != "zero_run_first")
    if profile == "zero_run_first":
        return [0, 0] + c
    if profile == "zero_run_last":
        return c + [0] * int(rng.integers(1, 3))
    first = 2 if c[0] == 0 else 1                                         # the inserted zero gets positive neighbours
    parity = 1 if profile == "zero_1run_inside" else 0
    places = [i for i in range(first, len(c)) if i % 2 == parity and i >= 1 + (parity == 0)]
    c.insert(int(rng.choice(places)), 0)
    return c


def same_mask_with_zero_runs(rng, counts):
    """A count list of the same mask that no encoder writes: runs split as (a, 0, b) and pairs of zero-length runs put in, parity kept"""
    c = [int(v) for v in counts]
    for _ in range(int(rng.integers(1, 4))):
        i = int(rng.integers(0, len(c) + 1))
        if i < len(c) and rng.integers(0, 2):
            a = int(rng.integers(0, c[i] + 1))
            c[i:i + 1] = [a, 0, c[i] - a]
        else:
            c[i:i] = [0, 0]
    return c


def build_rle_counts(profile, seed):
    """M (3..12) count lists of one h x w (1..90 each; enough pixels for the profile's runs), any non-negative counts that add up to h * w: the first one or
    two are planted with the profile's zero runs, the next is the first with a zero-length 0-run put in front (its complement), the rest are canonical
    encodings of random run structure -- among them copies of the planted masks' canonical form, so a zero-run list meets its own plain twin.
    pairs [P, 3] = (a, b, crowd): every list with itself, the first with its complement and with its twin, random others.
    (The issue's range for M starts at 2; a case always holds a planted list, its complement and its twin, so M starts at 3.)"""
    assert profile in RLE_COUNTS_PROFILES
    rng = _rng("rle_counts", profile, seed)
    need = {"more_than_256_runs_with_zeros": 2 * PREFIX_ROUND + 60, "only_zero_runs_then_full": 1}.get(profile, 4)
    h = int(rng.integers(-(-need // 90), 91))                  # tall enough that some width up to 90 holds the profile's runs
    w = int(rng.integers(-(-need // h), 91))
    P = h * w
    M = int(rng.integers(3, 13))
    lists = [_plant(rng, profile, P)]
    if M >= 5:
        lists.append(_plant(rng, profile, P))
    n_planted = len(lists)
    lists.append([0] + lists[0])                                           # a zero-length 0-run in front flips every later run: the complement
    twin = cocoeval_ref.dense(lists[0], h, w)
    from isegmi import coco
    lists.append(coco.rle_counts(twin))                                    # the same mask, canonical
    while len(lists) < M:
        lists.append(_canonical_counts(rng, P, int(rng.integers(1, min(P, 40) + 1)), leading_one=bool(rng.integers(0, 2))) if P > 1 else [P])
    lists = lists[:max(M, n_planted + 2)]
    M = len(lists)
    pairs = [(i, i, 0) for i in range(M)] + [(0, n_planted, 0), (n_planted, 0, 1), (0, n_planted + 1, 0), (n_planted + 1, 0, 1)]
    pairs += [(int(a), int(b), int(c)) for a, b, c in zip(rng.integers(0, M, 3 * M), rng.integers(0, M, 3 * M), rng.integers(0, 2, 3 * M))]
    reached = set()
    for c in lists[:n_planted]:
        reached |= rle_conditions(c)
    return dict(op="rle_counts", profile=profile, seed=seed, h=h, w=w, counts=lists, planted=list(range(n_planted)), complement=(0, n_planted), twin=(0, n_planted + 1),
                pairs=np.array(pairs, np.int32), reached=reached)


def _bbox_xyxy(m):
    x, y, bw, bh = cocoeval_ref.tight_box(m)
    return [int(x), int(y), int(x + bw) - 1, int(y + bh) - 1]      # the device's form: inclusive corners, (0, 0, -1, -1) when empty


def ref_rle_counts(case):
    dense = [cocoeval_ref.dense(c, case["h"], case["w"]) for c in case["counts"]]
    return dict(area=np.array([int(d.sum()) for d in dense], np.int64), bbox=np.array([_bbox_xyxy(d) for d in dense], np.int32),
                iou=np.array([cocoeval_ref.mask_iou(dense[a], dense[b], bool(c)) for a, b, c in case["pairs"].tolist()], np.float64))


# ============================================================================================================ rle_encode, then RleSet / rle_iou on its counts
RLE_CHAIN_PROFILES = ("window_on_last_row", "window_on_chunk_border", "invalid_between_valid", "empty_and_full", "column_wrap")
RLE_CHUNK = 64          # rle.hip walks a column in chunks of 64 rows


def build_rle_chain(profile, seed):
    """masks [N, K, h, w] (N 1..3, K 1..5, h, w 1..200) with `count`, `image_hw` and `windows` present or absent by the seed, forced where the profile
    needs them.  `clean` is what is encoded; `masks` carries garbage bytes outside every window (when there are windows) and in every invalid slot.
    A slot's content lies inside its window; a window is (x0, y0, x1, y1), ends exclusive.
      window_on_last_row      slot (0, c - 1), the last valid one of image 0 with c < K: its window ends on the image's last row and reaches the last
                              column, the pixel in that corner set; the slot after it is invalid and full of garbage
      window_on_chunk_border  h > 64: a window whose y1 is 64 (or 128) with its last row set, another whose y0 is 64
      invalid_between_valid   N >= 2, count[0] < K, count[1] > 0: slots without runs lie between slots with runs
      empty_and_full          an all-clear and an all-set slot side by side (full: counts [0, h * w])
      column_wrap             the last row of a column and the first row of the next one set: one run crosses the column end"""
    assert profile in RLE_CHAIN_PROFILES
    rng = _rng("rle_chain", profile, seed)
    N, K = int(rng.integers(1, 4)), int(rng.integers(1, 6))
    h, w = int(rng.integers(1, 201)), int(rng.integers(1, 201))
    use_count, use_hw, use_win = (bool(v) for v in rng.integers(0, 2, 3))
    if profile == "window_on_last_row":
        K, use_count, use_win = max(K, 2), True, True
    elif profile == "window_on_chunk_border":
        h, use_win = int(rng.integers(RLE_CHUNK + 2, 201)), True
    elif profile == "invalid_between_valid":
        N, K, use_count = max(N, 2), max(K, 2), True
    elif profile == "empty_and_full":
        K = max(K, 2)
    elif profile == "column_wrap":
        w = max(w, 2)
    count = rng.integers(0, K + 1, N).astype(np.int32)
    count[0] = max(count[0], 1)
    if profile == "window_on_last_row":
        count[0] = int(rng.integers(1, K))
    elif profile == "invalid_between_valid":
        count[0], count[1] = int(rng.integers(1, K)), int(rng.integers(1, K + 1))
    elif profile == "empty_and_full":
        count[0] = max(count[0], 2)
    if not use_count:
        count[:] = K
    hw = np.stack([rng.integers(1, h + 1, N), rng.integers(1, w + 1, N)], 1).astype(np.int32)
    if profile == "window_on_chunk_border":
        hw[0, 0] = int(rng.integers(RLE_CHUNK + 1, h + 1))
    elif profile == "column_wrap":
        hw[0, 1] = max(hw[0, 1], 2)
    if not use_hw:
        hw[:] = (h, w)
    clean = np.zeros((N, K, h, w), np.uint8)
    wins = np.zeros((N, K, 4), np.int32)
    for n in range(N):
        hi, wi = int(hw[n, 0]), int(hw[n, 1])
        for k in range(K):
            x0, x1 = np.sort(rng.integers(0, wi + 1, 2)); y0, y1 = np.sort(rng.integers(0, hi + 1, 2))
            kind = int(rng.integers(0, 4))
            if kind == 0:
                x0, y0, x1, y1 = 0, 0, wi, hi
            wins[n, k] = (x0, y0, x1, y1)
            if x1 > x0 and y1 > y0:
                dens = (0.5, 0.95, 0.1, 1.0)[int(rng.integers(0, 4))]
                clean[n, k, y0:y1, x0:x1] = rng.uniform(0, 1, (y1 - y0, x1 - x0)) < dens
    h0, w0 = int(hw[0, 0]), int(hw[0, 1])

    def window(n, k, x0, y0, x1, y1, fill):
        clean[n, k] = 0
        wins[n, k] = (x0, y0, x1, y1)
        clean[n, k, y0:y1, x0:x1] = rng.uniform(0, 1, (y1 - y0, x1 - x0)) < fill
    if profile == "window_on_last_row":
        k = int(count[0]) - 1
        window(0, k, int(rng.integers(0, w0)), int(rng.integers(0, h0)), w0, h0, 0.7)
        clean[0, k, h0 - 1, w0 - 1] = 1
    elif profile == "window_on_chunk_border":
        y1 = RLE_CHUNK * int(rng.integers(1, (h0 - 1) // RLE_CHUNK + 1))
        window(0, 0, int(rng.integers(0, w0)), int(rng.integers(0, y1)), w0, y1, 0.7)
        clean[0, 0, y1 - 1, wins[0, 0, 0]:w0] = 1
        if count[0] > 1:
            window(0, 1, 0, RLE_CHUNK, int(rng.integers(1, w0 + 1)), h0, 0.7)
            clean[0, 1, RLE_CHUNK, 0] = 1
    elif profile == "empty_and_full":
        a = int(rng.integers(0, count[0] - 1))
        clean[0, a] = 0
        clean[0, a + 1] = 0
        clean[0, a + 1, :h0, :w0] = 1
        wins[0, a + 1] = (0, 0, w0, h0)
        if rng.integers(0, 2):
            wins[0, a] = (int(w0 // 2), int(h0 // 2), int(w0 // 2), int(h0 // 2))     # an empty window for the empty mask
    elif profile == "column_wrap":
        x = int(rng.integers(0, w0 - 1))
        x0 = int(rng.integers(0, x + 1))
        window(0, 0, x0, 0, int(rng.integers(x + 2, w0 + 1)), h0, 0.3)
        clean[0, 0, h0 - 1, x] = 1
        clean[0, 0, 0, x + 1] = 1
    masks = clean.copy()
    for n in range(N):
        for k in range(K):
            g = rng.integers(1, 256, (h, w)).astype(np.uint8)
            if k >= count[n]:
                masks[n, k] = g                                                        # an invalid slot is never read
            elif use_win:
                x0, y0, x1, y1 = wins[n, k]
                g[y0:y1, x0:x1] = clean[n, k, y0:y1, x0:x1]
                masks[n, k] = g
    valid = [(n, k) for n in range(N) for k in range(K) if k < count[n]]
    by_image = {}
    for i, (n, k) in enumerate(valid):
        by_image.setdefault(n, []).append(i)
    pairs = []
    for _ in range(3 * len(valid)):                                                     # pairs of slots of one image (one size), crowd or not
        ids = by_image[valid[int(rng.integers(0, len(valid)))][0]]
        pairs.append((int(rng.choice(ids)), int(rng.choice(ids)), int(rng.integers(0, 2))))
    reached = set()
    c0 = int(count[0])
    enc = lambda n, k: clean[n, k, :hw[n, 0], :hw[n, 1]]       # noqa: E731
    if use_win and use_count and c0 < K and tuple(wins[0, c0 - 1, 2:]) == (w0, h0) and enc(0, c0 - 1)[-1, -1] and (masks[0, c0] != 0).all():
        reached.add("window_on_last_row")
    if use_win and any(wins[n, k, 3] % RLE_CHUNK == 0 and wins[n, k, 3] > wins[n, k, 1] and wins[n, k, 2] > wins[n, k, 0]
                       and enc(n, k)[wins[n, k, 3] - 1, wins[n, k, 0]:wins[n, k, 2]].any() for n, k in valid):
        reached.add("window_on_chunk_border")
    if use_count and any(count[n] < K and count[n + 1:].any() for n in range(N - 1)):
        reached.add("invalid_between_valid")
    if any(not enc(n, k).any() and (n, k + 1) in valid and enc(n, k + 1).all() for n, k in valid):
        reached.add("empty_and_full")
    if any((enc(n, k)[-1, :-1] & enc(n, k)[0, 1:]).any() for n, k in valid if hw[n, 1] > 1):
        reached.add("column_wrap")
    return dict(op="rle_chain", profile=profile, seed=seed, masks=masks, clean=clean, count=count if use_count else None, image_hw=hw if use_hw else None,
                windows=wins if use_win else None, hw=hw, valid=valid, pairs=np.array(pairs, np.int32).reshape(-1, 3), reached=reached)


def ref_rle_chain(case):
    """per valid slot the oracle's counts and string; per pair the dense IoU; per slot area and tight box"""
    from oracle import ora
    hw = case["hw"]
    dense = [case["clean"][n, k, :hw[n, 0], :hw[n, 1]].astype(bool) for n, k in case["valid"]]
    counts = [ora.rle_encode(d) for d in dense]
    return dict(counts=counts, strings=[ora.rle_to_string(c) for c in counts], area=np.array([int(d.sum()) for d in dense], np.int64),
                bbox=np.array([_bbox_xyxy(d) for d in dense], np.int32).reshape(-1, 4),
                iou=np.array([cocoeval_ref.mask_iou(dense[a], dense[b], bool(c)) for a, b, c in case["pairs"].tolist()], np.float64))


# ============================================================================================================ pose_handoff
POSE_HANDOFF_PROFILES = ("score_tie_at_K", "at_person_thresh", "none_pass", "more_than_K")


def build_pose_handoff(profile, seed):
    """N 1..3 images, cap 1..12 detection slots, K 1..8 persons kept; scores and keypoint scores are multiples of 1/8, the thresholds too, so `>` against
    `>=` shows; slots at or beyond count[n] hold NaN.  Image 0 carries the profile's condition:
      score_tie_at_K    more candidates than K, and the K-th and (K+1)-th best hold the same score (cap > K)
      at_person_thresh  a slot whose score IS the threshold (strict `>`: not a candidate)
      none_pass         count > 0 and no candidate, next to an image that has some when N > 1
      more_than_K       more candidates than K"""
    assert profile in POSE_HANDOFF_PROFILES
    rng = _rng("pose_handoff", profile, seed)
    N, cap, K = int(rng.integers(1, 4)), int(rng.integers(1, 13)), int(rng.integers(1, 9))
    if profile in ("score_tie_at_K", "more_than_K"):
        cap = max(cap, 2)
        K = min(K, cap - 1)
    pt, kt = float(rng.integers(1, 6)) / 8.0, float(rng.integers(0, 5)) / 8.0
    score = (rng.integers(0, 9, (N, cap)) / 8.0).astype(F)
    count = rng.integers(0, cap + 1, N).astype(np.int32)
    if profile in ("score_tie_at_K", "more_than_K"):
        count[0] = int(rng.integers(K + 1, cap + 1))
        score[0, :count[0]] = (rng.integers(int(pt * 8) + 1, 9, count[0]) / 8.0).astype(F)          # every one a candidate
        if profile == "score_tie_at_K":
            order = pose_handoff_ref.select(score[0], count[0], pt, cap)
            score[0, order[K]] = score[0, order[K - 1]]
    elif profile == "at_person_thresh":
        count[0] = max(count[0], 1)
        score[0, int(rng.integers(0, count[0]))] = F(pt)
    elif profile == "none_pass":
        count[0] = max(count[0], 1)
        score[0] = (rng.integers(0, int(pt * 8) + 1, cap) / 8.0).astype(F)
        if N > 1:
            count[1] = max(count[1], 1)
            score[1, 0] = F(1.0)
    kpt = np.zeros((N, cap, 17, 3), F)
    kpt[..., 0] = rng.integers(0, 4 * 640, (N, cap, 17)) / 4.0
    kpt[..., 1] = rng.integers(0, 4 * 480, (N, cap, 17)) / 4.0
    kpt[..., 2] = 1.0
    kscore = (rng.integers(0, 9, (N, cap, 17)) / 8.0).astype(F)
    for n in range(N):
        score[n, count[n]:] = np.nan; kpt[n, count[n]:] = np.nan; kscore[n, count[n]:] = np.nan
    ratios = (rng.integers(3, 12, (N, 2)) / rng.integers(3, 12, (N, 2))).astype(F)
    s0, c0 = score[0, :count[0]], int(count[0])
    ncand = int((s0 > F(pt)).sum())
    reached = set()
    if ncand > K:
        reached.add("more_than_K")
        top = np.sort(s0[s0 > F(pt)])[::-1]
        if top[K - 1] == top[K]:
            reached.add("score_tie_at_K")
    if (s0 == F(pt)).any():
        reached.add("at_person_thresh")
    if c0 > 0 and ncand == 0:
        reached.add("none_pass")
    return dict(op="pose_handoff", profile=profile, seed=seed, reached=reached,
                args=dict(score=score, count=count, kpt=kpt, kscore=kscore, ratios=ratios, person_thresh=pt, kp_thresh=kt, K=K))


def ref_pose_handoff(case):
    kp, sc, sl, cnt = pose_handoff_ref.handoff(**case["args"])
    return dict(kpts=kp, score=sc, slot=sl, count=cnt)


# ============================================================================================================ keypoint_decode
KEYPOINT_PROFILES = ("argmax_tie", "subpixel_box", "huge_box", "count_zero", "peak_on_border")
KEYPOINT_THREADS = 256   # the decode kernel's block: min(wc, 256) columns, 256 // columns row segments


def build_keypoint_decode(profile, seed):
    """N 1..3 images of cap 1..6 slots, K in {1, 17} channels, heat maps of side S 2..12 holding multiples of 1/4; boxes have quarter-pixel corners and
    resized sides up to 40, except as the profile says.  Slots at or beyond count[n] hold NaN maps and boxes.  Slot (0, 0) carries the condition:
      argmax_tie      the box resizes the map onto itself (both sides S: every bicubic weight is exactly 0 or 1) and the map's maximum is planted twice
                      per channel (or the map is flat): the first in row-major order wins
      subpixel_box    a box narrower and lower than one pixel (sides < 1 count as 1): a 1 x 1 or 1 x n resize
      huge_box        a resized width past 256 (the second stride of columns) and a height past the segments' rows; K = 1 keeps the restatement quick
                      (measured: 9 ms for a 300 x 90 box at K = 1)
      count_zero      image 0 has no detection at all, next to one that has (N >= 2)
      peak_on_border  one side of the box is S (that axis is the identity) and the first or last row / column of the map holds values >= 8 against
                      <= 1 elsewhere: bicubic weights add up to 1 with negative lobes of at most 0.21, so the arg-max lies on that border"""
    assert profile in KEYPOINT_PROFILES
    rng = _rng("keypoint_decode", profile, seed)
    N, cap, K, S = int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.choice([1, 17])), int(rng.integers(2, 13))
    if profile == "huge_box":
        K = 1
    if profile == "count_zero":
        N = max(N, 2)
    heat = (rng.integers(-8, 9, (N * cap, S, S, K)) / 4.0).astype(F)
    x1 = rng.integers(0, 400, (N, cap)) / 4.0; y1 = rng.integers(0, 400, (N, cap)) / 4.0
    bw = rng.integers(1, 160, (N, cap)) / 4.0; bh = rng.integers(1, 160, (N, cap)) / 4.0
    boxes = np.stack([x1, y1, x1 + bw, y1 + bh], -1).astype(F)
    count = rng.integers(0, cap + 1, N).astype(np.int32)
    count[0] = max(count[0], 1)
    border = None
    if profile == "argmax_tie":
        boxes[0, 0, 2:] = boxes[0, 0, :2] + F(S) - (rng.integers(0, 4, 2) / 4.0).astype(F)          # ceil(side) = S
        for k in range(K):
            a, b = rng.choice(S * S, 2, replace=False) if S * S > 1 else (0, 0)
            heat[0].reshape(S * S, K)[[a, b], k] = 2.5
            if rng.integers(0, 4) == 0:
                heat[0, :, :, k] = 0.75                                                              # a flat map: position 0
    elif profile == "subpixel_box":
        boxes[0, 0, 2:] = boxes[0, 0, :2] + (rng.integers(0, 4, 2) / 4.0).astype(F)                 # sides 0 .. 0.75
        if cap > 1 and count[0] > 1:
            boxes[0, 1, 2] = boxes[0, 1, 0] - F(3.0)                                                 # an inverted box: a negative width counts as 1 too
    elif profile == "huge_box":
        boxes[0, 0, 2] = boxes[0, 0, 0] + F(int(rng.integers(KEYPOINT_THREADS + 1, 321))) - F(0.25)
        boxes[0, 0, 3] = boxes[0, 0, 1] + F(int(rng.integers(2, 91)))
    elif profile == "count_zero":
        count[0], count[1] = 0, max(count[1], 1)
    elif profile == "peak_on_border":
        axis, last = int(rng.integers(0, 2)), bool(rng.integers(0, 2))
        heat[0] = (rng.integers(-4, 5, (S, S, K)) / 4.0).astype(F)
        line = (rng.integers(32, 37, (S, K)) / 4.0).astype(F)
        if axis == 0:
            heat[0, S - 1 if last else 0, :, :] = line
            boxes[0, 0, 3] = boxes[0, 0, 1] + F(S)
        else:
            heat[0, :, S - 1 if last else 0, :] = line
            boxes[0, 0, 2] = boxes[0, 0, 0] + F(S)
        border = (axis, last)
    for n in range(N):
        boxes[n, count[n]:] = np.nan
        heat[n * cap + count[n]:(n + 1) * cap] = np.nan
    reached = set()
    if count[0] > 0:
        w, h, wc, hc = keypoint_ref.box_sizes(boxes[0, 0])
        if (wc, hc) == (S, S) and all((heat[0, :, :, k] == heat[0, :, :, k].max()).sum() >= 2 for k in range(K)):
            reached.add("argmax_tie")
        if boxes[0, 0, 2] - boxes[0, 0, 0] < 1 and boxes[0, 0, 3] - boxes[0, 0, 1] < 1:
            reached.add("subpixel_box")
        if wc > KEYPOINT_THREADS and hc > 1:
            reached.add("huge_box")
        if border is not None and (hc if border[0] == 0 else wc) == S:
            reached.add("peak_on_border")
    if count[0] == 0 and count[1:].any():
        reached.add("count_zero")
    return dict(op="keypoint_decode", profile=profile, seed=seed, heat=heat, boxes=boxes, count=count, border=border, reached=reached)


def ref_keypoint_decode(case):
    with np.errstate(invalid="ignore"):
        kpt, ks = keypoint_ref.decode(case["heat"], case["boxes"], case["count"])
    return dict(kpt=kpt, kscore=ks)


# ============================================================================================================ paint
PAINT_PROFILES = ("outline_off_image", "dot_off_image", "everything_on_one_pixel", "slot_minus_one_only", "width_not_multiple_of_4")


def build_paint(profile, seed):
    """An H x W image (H 1..40, W 1..300), `slots` 1..5 mask planes of (ph, pw) = render_ref.plane_shape(H, W, pw_extra in {0, 1, 3}) holding the bytes
    0 / 1 / 2 / 255, D 0..40 entries and Q 0..60 dots (half 0..8).  Corners and dot centres reach a few pixels past every edge in every profile.
      outline_off_image        D >= 4: outlines with corners left / above the image, past its right / bottom edge, and inverted (x2 < x1, y2 < y1)
      dot_off_image            Q >= 4: dot centres outside the image, one pixel out of reach (half + 1 away) and just in reach (half away)
      everything_on_one_pixel  every entry and every dot touches one pixel (render_ref.overlap_case plus dots over it)
      slot_minus_one_only      every entry has slot -1 (boxes only; the planes are there and must not show)
      width_not_multiple_of_4  W % 4 != 0 (a thread paints four pixels): the last group of a row is partial"""
    assert profile in PAINT_PROFILES
    rng = _rng("paint", profile, seed)
    H, W = int(rng.integers(1, 41)), int(rng.integers(1, 301))
    pw_extra, slots = int(rng.choice([0, 1, 3])), int(rng.integers(1, 6))
    D, Q = int(rng.integers(0, 41)), int(rng.integers(0, 61))
    if profile == "width_not_multiple_of_4" and W % 4 == 0:
        W += int(rng.integers(1, 4))
    if profile == "outline_off_image":
        D = max(D, 4)
    if profile == "dot_off_image":
        Q = max(Q, 4)
    if profile == "everything_on_one_pixel":
        D, Q = max(D, 2), max(Q, 2)
        image, masks, e, (cx, cy) = render_ref.overlap_case(int(rng.integers(0, 2 ** 31)), H, W, pw_extra, D, slots)
    else:
        ph, pw = render_ref.plane_shape(H, W, pw_extra)
        image = render_ref.random_image(rng, H, W)
        masks = render_ref.VALUES[rng.integers(0, 4, (slots, ph, pw))]
        e = np.zeros((D, 8), np.int32)
        e[:, 0] = rng.integers(-1, slots, D)
        e[:, 1] = rng.integers(-3, W + 3, D); e[:, 3] = rng.integers(-3, W + 3, D)
        e[:, 2] = rng.integers(-3, H + 3, D); e[:, 4] = rng.integers(-3, H + 3, D)
        e[:, 5] = rng.integers(0, 1 << 24, D)
        e[:, 6] = rng.integers(0, 2, D)
    d = np.zeros((Q, 4), np.int32)
    d[:, 0] = rng.integers(-10, W + 10, Q); d[:, 1] = rng.integers(-10, H + 10, Q)
    d[:, 2] = rng.integers(0, 1 << 24, Q); d[:, 3] = rng.integers(0, 9, Q)
    if profile == "outline_off_image":
        e[0, 1:5] = (-int(rng.integers(1, 6)), -int(rng.integers(1, 5)), int(rng.integers(0, W)), int(rng.integers(0, H)))
        e[1, 1:5] = (int(rng.integers(0, W)), int(rng.integers(0, H)), W + int(rng.integers(0, 4)), H + int(rng.integers(0, 4)))
        e[2, 1:5] = (W - 1, H - 1, 0, 0) if rng.integers(0, 2) else (W + 1, int(rng.integers(0, H)), -2, int(rng.integers(0, H)))
        e[3, 1:5] = (-1, -1, W, H)
        e[:4, 6] = 1
    elif profile == "dot_off_image":
        half = rng.integers(0, 9, 4)
        d[0] = (-int(half[0]) - 1, int(rng.integers(0, H)), 0xFF0000, half[0])        # one pixel out of reach on the left
        d[1] = (W + int(half[1]) - 1, int(rng.integers(0, H)), 0x00FF00, half[1])     # its left edge is the last column
        d[2] = (int(rng.integers(0, W)), -int(half[2]), 0x0000FF, half[2])            # its bottom edge is row 0
        d[3] = (int(rng.integers(0, W)), H + int(half[3]), 0xFFFFFF, half[3])         # one pixel out of reach below
    elif profile == "everything_on_one_pixel":
        d[:, 3] = rng.integers(0, 9, Q)
        d[:, 0] = cx + rng.integers(-8, 9, Q).clip(-d[:, 3], d[:, 3])
        d[:, 1] = cy + rng.integers(-8, 9, Q).clip(-d[:, 3], d[:, 3])
    elif profile == "slot_minus_one_only":
        D = max(D, 1)
        if len(e) == 0:
            e = np.array([[0, 0, 0, W - 1, H - 1, 0x123456, 1, 0]], np.int32)
        e[:, 0] = -1
        e[0, 6] = 1
    reached = set()
    on = e[(e[:, 6] & 1) == 1]
    if len(on) and (on[:, 1] < 0).any() and (on[:, 2] < 0).any() and (on[:, 3] >= W).any() and (on[:, 4] >= H).any() and ((on[:, 3] < on[:, 1]) | (on[:, 4] < on[:, 2])).any():
        reached.add("outline_off_image")
    if len(d) and ((d[:, 0] < 0) | (d[:, 0] >= W) | (d[:, 1] < 0) | (d[:, 1] >= H)).any() and (-d[:, 0] == d[:, 3] + 1).any() and (d[:, 0] - (W - 1) == d[:, 3]).any():
        reached.add("dot_off_image")
    if profile == "everything_on_one_pixel":
        touch_e = all((s >= 0 and masks[s, cy, cx]) or (f & 1 and x1 == cx and y1 <= cy <= y2) for s, x1, y1, x2, y2, _, f, _ in e.tolist())
        touch_d = all(abs(x - cx) <= hf and abs(y - cy) <= hf for x, y, _, hf in d.tolist())
        if touch_e and touch_d:
            reached.add("everything_on_one_pixel")
    if len(e) and (e[:, 0] == -1).all():
        reached.add("slot_minus_one_only")
    if W % 4:
        reached.add("width_not_multiple_of_4")
    return dict(op="paint", profile=profile, seed=seed, image=image, masks=masks, entries=e, dots=d, reached=reached)


def ref_paint(case):
    return dict(image=render_ref.paint_ref(case["image"], case["masks"], case["entries"], case["dots"]))


# ============================================================================================================ resample_u8
RESAMPLE_PROFILES = ("one_axis_identity", "up_one_axis_down_other", "rows_cross_chunk", "image_smaller_than_tile_in_canvas", "one_by_one")
RESAMPLE_TILE_H, RESAMPLE_TILE_W, RESAMPLE_CHUNK = 16, 64, 32      # resample.hip: output tile, source rows per LDS chunk (tests/test_resample_ops_gpu.py)
RESAMPLE_MEAN = (102.9801, 115.9465, 122.7717)


def resample_tile_rows(h, oh):
    """source rows the first output tile of an h -> oh resize reads"""
    b, _ = resample_ref.coeffs(h, oh)
    last = min(oh, RESAMPLE_TILE_H) - 1
    return int(b[last, 0] + b[last, 1] - b[0, 0])


def build_resample(profile, seed):
    """1..4 images (h, w 1..80) and one view of each, (oh, ow) 1..80, mirrored or not, each on its own plane of a canvas of at most 96 x 160 at a random
    (dst_y, dst_x); the same entries serve both epilogues (the byte one ignores the placement).  View 0 carries the condition:
      one_axis_identity                  oh == h and ow != w, or the other way round: one pass is skipped
      up_one_axis_down_other             one axis grows, the other shrinks
      rows_cross_chunk                   h >= 40 and 16 <= oh <= h / 2: the first tile reads more than 32 source rows (two LDS chunks or more), while
                                         the columns stay inside one chunk's width -- the two axes fall on different sides
      image_smaller_than_tile_in_canvas  oh < 16 and ow < 64, placed off the canvas's origin with padding all round
      one_by_one                         a 1 x 1 source, or a 1 x 1 output, by the seed"""
    assert profile in RESAMPLE_PROFILES
    rng = _rng("resample", profile, seed)
    n = int(rng.integers(1, 5))
    shapes = [(int(rng.integers(1, 81)), int(rng.integers(1, 81))) for _ in range(n)]
    outs = [(int(rng.integers(1, 81)), int(rng.integers(1, 81))) for _ in range(n)]
    h, w = shapes[0]
    oh, ow = outs[0]
    if profile == "one_axis_identity":
        if rng.integers(0, 2):
            oh, ow = h, (ow if ow != w else w % 80 + 1)
        else:
            ow, oh = w, (oh if oh != h else h % 80 + 1)
    elif profile == "up_one_axis_down_other":
        h, w = int(rng.integers(2, 80)), int(rng.integers(2, 80))
        if rng.integers(0, 2):
            oh, ow = int(rng.integers(h + 1, 81)), int(rng.integers(1, w))
        else:
            oh, ow = int(rng.integers(1, h)), int(rng.integers(w + 1, 81))
    elif profile == "rows_cross_chunk":
        h = int(rng.integers(40, 81))
        oh = int(rng.integers(RESAMPLE_TILE_H, h // 2 + 1))
    elif profile == "image_smaller_than_tile_in_canvas":
        oh, ow = int(rng.integers(1, RESAMPLE_TILE_H)), int(rng.integers(1, RESAMPLE_TILE_W))
    elif profile == "one_by_one":
        if rng.integers(0, 2):
            h, w = 1, 1
        else:
            oh, ow = 1, 1
    shapes[0], outs[0] = (h, w), (oh, ow)
    images = []
    for i, (a, b) in enumerate(shapes):
        kind = int(rng.integers(0, 3))
        images.append(list(resample_ref.patterns(a, b, int(rng.integers(0, 2 ** 31))).values())[kind])
    Hp = int(rng.integers(max(o[0] for o in outs) + (2 if profile == "image_smaller_than_tile_in_canvas" else 0), 97))
    Wp = int(rng.integers(max(o[1] for o in outs) + (2 if profile == "image_smaller_than_tile_in_canvas" else 0), 161))
    entries = []
    for i, (a, b) in enumerate(outs):
        dy, dx = int(rng.integers(0, Hp - a + 1)), int(rng.integers(0, Wp - b + 1))
        if i == 0 and profile == "image_smaller_than_tile_in_canvas":
            dy, dx = int(rng.integers(1, Hp - a)), int(rng.integers(1, Wp - b))
        entries.append((i, a, b, dy, dx, int(rng.integers(0, 2)), i))
    swap, fill = bool(rng.integers(0, 2)), float(rng.choice([0.0, 0.5, -3.0]))
    mean, std = (RESAMPLE_MEAN, (1.0, 1.0, 1.0)) if rng.integers(0, 2) else ((0.0, 0.0, 0.0), (255.0, 255.0, 255.0))
    _, oh, ow, dy, dx, _, _ = entries[0]
    reached = set()
    if (oh == h) != (ow == w):
        reached.add("one_axis_identity")
    if (oh > h and ow < w) or (oh < h and ow > w):
        reached.add("up_one_axis_down_other")
    if resample_tile_rows(h, oh) > RESAMPLE_CHUNK:
        reached.add("rows_cross_chunk")
    if oh < RESAMPLE_TILE_H and ow < RESAMPLE_TILE_W and 0 < dy and dy + oh < Hp and 0 < dx and dx + ow < Wp:
        reached.add("image_smaller_than_tile_in_canvas")
    if (h, w) == (1, 1) or (oh, ow) == (1, 1):
        reached.add("one_by_one")
    return dict(op="resample", profile=profile, seed=seed, images=images, entries=entries, canvas=(Hp, Wp), mean=mean, std=std, swap=swap, fill=fill, reached=reached)


def ref_resample(case):
    Hp, Wp = case["canvas"]
    views = [resample_ref.resize_view(case["images"][i], oh, ow, bool(flip)) for i, oh, ow, _, _, flip, _ in case["entries"]]
    canvas = np.stack([resample_ref.canvas_f32(case["images"][i], oh, ow, Hp, Wp, dy, dx, case["mean"], case["std"], case["swap"], case["fill"], bool(flip))
                       for i, oh, ow, dy, dx, flip, _ in case["entries"]])
    return dict(views=views, canvas=canvas)


OPS = {
    "rle_counts": (build_rle_counts, ref_rle_counts, RLE_COUNTS_PROFILES),
    "rle_chain": (build_rle_chain, ref_rle_chain, RLE_CHAIN_PROFILES),
    "pose_handoff": (build_pose_handoff, ref_pose_handoff, POSE_HANDOFF_PROFILES),
    "keypoint_decode": (build_keypoint_decode, ref_keypoint_decode, KEYPOINT_PROFILES),
    "paint": (build_paint, ref_paint, PAINT_PROFILES),
    "resample": (build_resample, ref_resample, RESAMPLE_PROFILES),
}


# ============================================================================================================ yolo_select
YOLO_PROFILES = ("slice_border", "tie_at_cut", "none_pass", "all_pass_over_top_n", "class_tie_single_label", "nan_inf_box", "min_wh_edge")
YOLO_SLICE_FLOATS = 8192      # csrc/yolo_ops.hip YOLO_SLICE: a block of the first launch takes 8192 // (5 + C) whole anchor records
YOLO_TOP_NS, YOLO_THRS = (1, 7, 64, 1024), (0.0, 0.05, 0.5)
YOLO_ON, YOLO_OFF = F(30.0), F(-30.0)     # sigmoid(30) is exactly 1.0; sigmoid(-30) = 9.4e-14


def _q(rng, lo, hi, shape, step=4.0):
    """multiples of 1 / step in [lo, hi]"""
    return (rng.integers(int(lo * step), int(hi * step) + 1, shape) / step).astype(F)


def build_yolo_select(profile, seed):
    """nl 1..3 levels of N 1..3 images, A 1..3 anchors, C in {1, 2, 5, 80}, grids 1..13 a side, top_n in {1, 7, 64, 1024}, thr in {0, 0.05, 0.5}, multi_label
    0 / 1, min_wh in {0, 2}.  Every logit is a multiple of 1/4 in [-4, 4], so equal scores are everywhere.  Row (level 0, image 0) carries the condition:
      slice_border            C = 80 and more than 96 records: the records on both sides of the first slice border hold candidates of one equal score
      tie_at_cut              top_n - 1 pairs at class logit 3, three at 2, the rest at -8 under one objectness: the top_n-th and the next candidate tie
                              (top_n is drawn among those the row can overflow: pairs with multi_label, records without)
      none_pass               no candidate (thr 0: objectness and classes at -inf, whose product underflows to 0, and 0 > 0 fails)
      all_pass_over_top_n     every pair (multi_label 0: every record's best) passes and there are more of them than top_n
      class_tie_single_label  multi_label 0, C >= 2: one record's best sigmoid is held by two classes (the lower wins), another's by logits 30 and 40,
                              both exactly 1.0 (a rule by logit would take the higher)
      nan_inf_box             candidates whose tx is NaN (dropped), tw +inf (the canvas's width), tw -inf (a side of 0), th NaN (dropped)
      min_wh_edge             min_wh 2 and an anchor of (2, 2): tx = ty = tw = th = 0 gives a box of sides exactly 2 (kept by >=), tw = -1/4 a narrower one
    When thr is 0.5 another row (if there is one) holds a pair of score exactly 0.5 (objectness 1.0, class logit 0), which `>` rejects."""
    import yolov3_ref
    assert profile in YOLO_PROFILES
    rng = _rng("yolo_select", profile, seed)
    nl, N, A = (int(v) for v in rng.integers(1, 4, 3))
    C = int(rng.choice([1, 2, 5, 80]))
    top_n, thr = int(rng.choice(YOLO_TOP_NS)), float(rng.choice(YOLO_THRS))
    ml, min_wh = int(rng.integers(0, 2)), float(rng.choice([0.0, 2.0]))
    grids = [(int(rng.integers(1, 14)), int(rng.integers(1, 14))) for _ in range(nl)]
    if profile == "slice_border":
        C, A, grids[0] = 80, max(A, 2), (int(rng.integers(7, 14)), int(rng.integers(7, 14)))
    elif profile == "class_tie_single_label":
        ml, C = 0, int(rng.choice([2, 5, 80]))
    elif profile == "min_wh_edge":
        min_wh = 2.0
    if grids[0][0] * grids[0][1] * A < 5:
        grids[0] = (int(rng.integers(2, 14)), int(rng.integers(3, 14)))
    H0, W0 = grids[0]
    nrec = H0 * W0 * A
    capacity = nrec * (C if ml else 1)
    if profile in ("tie_at_cut", "all_pass_over_top_n"):
        top_n = int(rng.choice([t for t in YOLO_TOP_NS if t + 2 <= capacity]))
    strides = yolov3_ref.STRIDES[:nl]
    anchors = yolov3_ref.ANCHORS[:nl, :A].copy()
    heads = []
    for H, W in grids:
        h = np.empty((N, H, W, A, 5 + C), F)
        h[..., :2] = _q(rng, -2, 2, (N, H, W, A, 2)); h[..., 2:4] = _q(rng, -1, 1, (N, H, W, A, 2)); h[..., 4:] = _q(rng, -4, 4, (N, H, W, A, 1 + C))
        heads.append(h)
    rec = heads[0][0].reshape(nrec, 5 + C)          # a view: the row's records
    if profile == "slice_border":
        rs = YOLO_SLICE_FLOATS // (5 + C)
        rec[:, 4:] = YOLO_OFF
        for j, r in enumerate(sorted({0, rs - 2, rs - 1, rs, rs + 1, nrec - 1})):
            rec[r, 4], rec[r, 5 + (7 * j) % C] = YOLO_ON, 1.0
    elif profile == "tie_at_cut":
        rec[:, 4], rec[:, 5:] = 4.0, -8.0
        if ml:
            flat = rng.choice(nrec * C, top_n + 2, replace=False)
        else:
            flat = rng.choice(nrec, top_n + 2, replace=False) * C + rng.integers(0, C, top_n + 2)
        rec[flat // C, 5 + flat % C] = np.where(np.arange(top_n + 2) < top_n - 1, F(3.0), F(2.0))
    elif profile == "none_pass":
        rec[:, 4:] = -np.inf if thr == 0.0 else YOLO_OFF
    elif profile == "all_pass_over_top_n":
        rec[:, 4] = _q(rng, 2, 4, nrec); rec[:, 5:] = _q(rng, 1, 4, (nrec, C))
    elif profile == "class_tie_single_label":
        r0, r1 = (int(v) for v in rng.choice(nrec, 2, replace=False))
        a, b = np.sort(rng.choice(C, 2, replace=False))
        rec[r0, 4], rec[r0, 5:] = 2.0, -2.0
        rec[r0, [5 + a, 5 + b]] = 1.5
        rec[r1, 4], rec[r1, 5:] = 1.0, -2.0
        rec[r1, 5 + a], rec[r1, 5 + b] = 30.0, 40.0
    elif profile == "nan_inf_box":
        plants = ((0, 0, np.inf, 0), (np.nan, 0, 0, 0), (0, 0, -np.inf, 0), (0, 0, 0, np.nan), (0, 0, 0, np.inf))
        for j, r in enumerate(rng.choice(nrec, len(plants), replace=False)):
            rec[r, :4] = plants[j]
            rec[r, 4], rec[r, 5 + j % C] = YOLO_ON, 1.0 + 0.25 * j
    elif profile == "min_wh_edge":
        anchors[0, 0] = (2.0, 2.0)
        cells = rng.choice(H0 * W0, 2, replace=False) * A          # anchor 0 of two cells
        rec[cells[0], :4], rec[cells[1], :4] = 0.0, (0.0, 0.0, -0.25, 0.0)
        rec[cells, 4], rec[cells, 5] = YOLO_ON, 2.0
    if thr == 0.5 and (N > 1 or nl > 1):
        other = heads[-1][N - 1].reshape(-1, 5 + C)
        r = int(rng.integers(0, len(other)))
        other[r, 4], other[r, 5:] = YOLO_ON, -4.0
        other[r, 5] = 0.0
    heads = [np.ascontiguousarray(h.reshape(N, h.shape[1], h.shape[2], -1)) for h in heads]
    canvas_w, canvas_h = max(s * g[1] for s, g in zip(strides, grids)), max(s * g[0] for s, g in zip(strides, grids))
    kw = dict(strides=strides, anchors=anchors, A=A, top_n=top_n, thr=thr, multi_label=bool(ml), min_wh=min_wh, canvas_w=canvas_w, canvas_h=canvas_h)
    # what the row holds, by the restatement's scores
    row = heads[0][0]
    rec = row.reshape(nrec, 5 + C)
    with np.errstate(invalid="ignore"):
        s = yolov3_ref.scores(row, A, bool(ml))
        cand = s > F(thr)
        p = yolov3_ref.sigmoid(rec[:, 5:])
    ncand = int(cand.sum())
    reached = set()
    rs = YOLO_SLICE_FLOATS // (5 + C)
    if nrec > rs and cand.reshape(nrec, C)[rs - 1].any() and cand.reshape(nrec, C)[rs].any():
        reached.add("slice_border")
    if ncand > top_n:
        v = np.sort(s[cand])[::-1]
        if v[top_n - 1] == v[top_n]:
            reached.add("tie_at_cut")
        if ncand == (s != -1).sum() == capacity:
            reached.add("all_pass_over_top_n")
    if ncand == 0:
        reached.add("none_pass")
    crec = cand.reshape(nrec, C).any(1)
    if not ml and C >= 2 and (crec & ((p == p.max(1, keepdims=True)).sum(1) >= 2)).any():
        reached.add("class_tie_single_label")
    if (crec & ~np.isfinite(rec[:, :4]).all(1)).any():
        reached.add("nan_inf_box")
    if min_wh > 0 and ncand:
        sc, idx, _ = yolov3_ref.select_level(row, A, 1 << 30, thr, bool(ml))
        b = yolov3_ref.decode_level(sc, idx, row, strides[0], anchors[0], canvas_w, canvas_h, A, 0.0)[0]
        if len(b) and ((b[:, 2] - b[:, 0] == F(min_wh)) | (b[:, 3] - b[:, 1] == F(min_wh))).any():
            reached.add("min_wh_edge")
    return dict(op="yolo_select", profile=profile, seed=seed, heads=heads, kw=kw, reached=reached)


def ref_yolo_select(case, **forks):
    import yolov3_ref
    dec, total = yolov3_ref.select_decode(case["heads"], **case["kw"], **forks)
    return dict(dec=dec, total=total)


# ============================================================================================================ retina_select / retina_postprocess
RETINA_PROFILES = ("tie_at_cut", "at_threshold", "empty_level", "cap_cut", "iou_at_threshold", "all_one_class")
RETINA_TOP_NS = (1, 50, 1000)


def _grid_anchor_boxes(rng, n):
    """integer boxes on a 10-pixel grid inside a 300 x 400 image (x2 <= 339, y2 <= 239: never clipped), sides 10 .. 50 counted with the +1"""
    x = rng.integers(0, 30, n) * 10.0; y = rng.integers(0, 20, n) * 10.0
    wh = rng.integers(1, 6, (n, 2)) * 10.0
    return np.stack([x, y, x + wh[:, 0] - 1, y + wh[:, 1] - 1], 1).astype(F)


def build_retina(profile, seed):
    """nl 1..5 levels, N 1..3 images, A in {1, 9}, C in {1, 2, 80}, grids 1..12 a side, top_n in {1, 50, 1000}; logits are multiples of 1/4 in [-6, 2] (a
    sigmoid of 0.05 lies between -3 and -2.75), thr 0.05 or 0.5 (sigmoid(0) is exactly 0.5).  Anchors are integer boxes on a 10-pixel grid; level 0 has zero
    deltas, so its decoded boxes ARE its anchors and their IoUs are simple fractions; the other levels have random deltas.  The postprocess takes the
    selected lists as the select stage left them (nseg = nl, seg_len = top_n), under random nms_flags 0..7, det_per_img in {1, 3, 20}.
    retina_postprocess holds nl * top_n <= 8192 slots: every combination of the ranges fits (5 * 1000).
      tie_at_cut        row (level 0, image 0): top_n - 1 logits at 1.5, three at 1, the rest at -6: the top_n-th and the next candidate tie
      at_threshold      thr 0.5 and logits of exactly 0 in the row: a score that IS the threshold is no candidate
      empty_level       nl >= 2: level 0 of image 0 has no candidate, the last level has
      cap_cut           the row holds det_per_img + 3 candidates on pairwise disjoint anchors in equal-score pairs: more survive the NMS than
                        det_per_img, and the kth-value cut keeps the ties at the cut
      iou_at_threshold  nms_thr 0.5 and two same-class pairs in the row: (0,0,9,9) / (0,0,9,4) has IoU 50 / 100 with the +1 areas, (0,0,10,10) /
                        (0,0,10,5) has 50 / 100 with plain areas -- whichever arithmetic nms_flags selects, one pair sits on the threshold
      all_one_class     every candidate of image 0 has one class"""
    import retinanet_ref
    assert profile in RETINA_PROFILES
    rng = _rng("retina", profile, seed)
    nl, N = int(rng.integers(1, 6)), int(rng.integers(1, 4))
    A, C = int(rng.choice([1, 9])), int(rng.choice([1, 2, 80]))
    top_n, thr = int(rng.choice(RETINA_TOP_NS)), float(rng.choice([0.05, 0.5]))
    det, flags = int(rng.choice([1, 3, 20])), int(rng.integers(0, 8))
    grids = [(int(rng.integers(1, 13)), int(rng.integers(1, 13))) for _ in range(nl)]
    if profile == "empty_level":
        nl = max(nl, 2)
        grids = (grids + [(int(rng.integers(1, 13)), int(rng.integers(1, 13)))])[:nl]
    if profile == "at_threshold":
        thr = 0.5
    if grids[0][0] * grids[0][1] * A < 24:
        grids[0] = (int(rng.integers(4, 13)), int(rng.integers(6, 13)))
    H0, W0 = grids[0]
    nrec = H0 * W0 * A
    if profile == "tie_at_cut":
        top_n = int(rng.choice([t for t in RETINA_TOP_NS if t + 2 <= nrec * C]))
    elif profile in ("cap_cut", "iou_at_threshold", "all_one_class"):
        top_n = int(rng.choice(RETINA_TOP_NS[1:]))            # the planted candidates all get through the select stage
    logits = [_q(rng, -6, 2, (N, H, W, A * C)) for H, W in grids]
    deltas = [np.zeros((N, H0, W0, A * 4), F)] + [rng.normal(0, 0.3, (N, H, W, A * 4)).astype(F) for H, W in grids[1:]]
    anchors = [_grid_anchor_boxes(rng, H * W * A) for H, W in grids]
    row = logits[0][0].reshape(nrec, C)            # a view
    hot = 1.0 if thr == 0.05 else 1.5              # passes either threshold
    nms_thr = 0.5 if profile == "iou_at_threshold" else float(rng.choice([0.4, 0.5]))
    if profile == "tie_at_cut":
        row[:] = -6.0
        flat = rng.choice(nrec * C, top_n + 2, replace=False)
        row.reshape(-1)[flat] = np.where(np.arange(top_n + 2) < top_n - 1, F(1.5), F(1.0))
    elif profile == "at_threshold":
        flat = rng.choice(nrec * C, min(4, nrec * C), replace=False)
        row.reshape(-1)[flat] = 0.0
    elif profile == "empty_level":
        row[:] = -6.0
        logits[-1][0].reshape(-1)[int(rng.integers(0, logits[-1][0].size))] = hot
    elif profile == "cap_cut":
        row[:] = -6.0
        m = det + 3
        r = rng.choice(nrec, m, replace=False)
        cell = rng.choice(30 * 20, m, replace=False)                                    # pairwise disjoint 10 x 10 boxes
        anchors[0][r] = np.stack([cell % 30 * 10.0, cell // 30 * 10.0, cell % 30 * 10.0 + 9, cell // 30 * 10.0 + 9], 1).astype(F)
        row[r, rng.integers(0, C, m)] = (1.0 + 0.25 * (np.arange(m) // 2)).astype(F)[::-1]     # equal-score pairs; the cut falls inside one
    elif profile == "iou_at_threshold":
        r = rng.choice(nrec, 4, replace=False)
        x, y = float(rng.integers(0, 28)) * 10.0, float(rng.integers(0, 20)) * 10.0
        anchors[0][r] = np.array([[x, y, x + 9, y + 9], [x, y, x + 9, y + 4], [x + 100, y, x + 110, y + 10], [x + 100, y, x + 110, y + 5]], F)
        c = int(rng.integers(0, C))
        row[:] = -6.0
        row[r, c] = (2.0, 1.75, 1.5, 1.25)
        for lg in logits[1:]:                                  # the pairs' class has no other candidate in the image: nothing else can suppress them
            lg[0].reshape(-1, C)[:, c] = -6.0
    elif profile == "all_one_class":
        c = int(rng.integers(0, C))
        for lg in logits:
            v = lg[0].reshape(-1, C)
            keep = v[:, c].copy()
            v[:] = -6.0
            v[:, c] = keep
        row[rng.choice(nrec, 6, replace=False), c] = hot
    hw = np.array([[300, 400], [280, 390], [300, 400]], np.int32)[:N]
    min_size = float(rng.choice([0.0, 25.0])) if profile not in ("cap_cut", "iou_at_threshold") else 0.0
    case = dict(op="retina", profile=profile, seed=seed, logits=logits, deltas=deltas, anchors=anchors, image_hw=hw, A=A, C=C, top_n=top_n, thr=thr, min_size=min_size,
                post=dict(nms_thr=nms_thr, det_per_img=det, cap=det + int(rng.integers(0, 4)), nms_flags=flags, ncls=C + 1))
    # what the case holds, from the restatement
    p = retinanet_ref.ora.map_f32(logits[0][0].reshape(-1), 1)
    cand = p > F(thr)
    reached = set()
    if cand.sum() > top_n:
        v = np.sort(p[cand])[::-1]
        if v[top_n - 1] == v[top_n]:
            reached.add("tie_at_cut")
    if (p == F(thr)).any():
        reached.add("at_threshold")
    if nl >= 2 and not cand.any() and (retinanet_ref.ora.map_f32(logits[-1][0].reshape(-1), 1) > F(thr)).any():
        reached.add("empty_level")
    want = ref_retina(case)
    if want["totals"][0] > det:
        reached.add("cap_cut")
    b, s, lb = want["lists"][0]
    plus = 0 if flags & 2 else 1
    same = lb[:, None] == lb[None, :]
    if len(b) > 1 and nms_thr == 0.5:
        area = (b[:, 2] - b[:, 0] + plus) * (b[:, 3] - b[:, 1] + plus)
        iw = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + plus, 0, None)
        ih = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + plus, 0, None)
        inter = (iw * ih).astype(np.float64)
        if (same & (2 * inter == area[:, None] + area[None, :] - inter) & (inter > 0) & ~np.eye(len(b), dtype=bool)).any():
            reached.add("iou_at_threshold")
    if len(lb) >= 2 and len(set(lb.tolist())) == 1:
        reached.add("all_one_class")
    return dict(case, reached=reached)


def ref_retina(case, **forks):
    """-> sel[l][n], dec[l][n], lists[n] (the concatenated candidate lists the postprocess takes), dets[n], totals[n]"""
    import retinanet_ref as rr
    N, nl = case["image_hw"].shape[0], len(case["logits"])
    sel = [[rr.select_level(lg[n], case["top_n"], case["thr"], **forks) for n in range(N)] for lg in case["logits"]]
    dec = [[rr.decode_level(*sel[l][n], case["deltas"][l][n], case["anchors"][l], case["image_hw"][n][1], case["image_hw"][n][0], case["C"], case["min_size"])
            for n in range(N)] for l in range(nl)]
    lists = [tuple(np.concatenate([d[n][k] for d in dec]) for k in range(3)) for n in range(N)]
    post = [rr.postprocess(*lists[n], return_total=True, **case["post"]) for n in range(N)]
    return dict(sel=sel, dec=dec, lists=lists, dets=[r[:3] for r in post], totals=[r[3] for r in post])


OPS.update({
    "yolo_select": (build_yolo_select, ref_yolo_select, YOLO_PROFILES),
    "retina": (build_retina, ref_retina, RETINA_PROFILES),
})


# ============================================================================================================ yolact_detect, nms_mode 0 / 1 / 2
YOLACT_PROFILES = ("empty_next_to_full", "identical_boxes", "iou_at_threshold", "class_tie", "over_top_k", "over_trad_cap", "P_below_wave")
YOLACT_MAX_SIZE = 512      # boxes are dyadic fractions of a 512-pixel canvas: decode with zero regressions and both IoU arithmetics are exact on them


def _px_priors(px):
    b = np.asarray(px, np.float64) / YOLACT_MAX_SIZE
    return np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(F)


def build_yolact_detect(profile, seed):
    """N 1..3 images of P 1..400 priors, ncls in {2, 5, 81}, 4 mask coefficients, trad_cap in {64, 128}, top_k in {10, 200}, max_det in {5, 100},
    conf_thresh 0.05, nms_thr 0.5.  Priors are boxes on an 8-pixel grid of a 512-pixel canvas (sides 8 .. 64) and the regressions are zero, so the decoded
    boxes are exact and IoUs are simple fractions.  Logits: background 0, foreground -12 except on `hot` priors, which carry one or two classes at
    multiples of 1/4 in [-2, 6] -- equal scores in different priors and classes are common.  One case serves the three nms modes.
      empty_next_to_full  N >= 2: image 0's background is at 30 (nothing passes the pre-filter), image 1 is crowded
      identical_boxes     every prior is the same box (P >= 2)
      iou_at_threshold    two pairs of one class: (0,0,16,16) / (0,0,16,8) has plain IoU 1/2 (modes 0, 1: `<=` keeps it), (0,0,3,3) / (0,0,3,1) has
                          (16, 8, 8) -> 1/2 with the +1 areas of mode 2 (`>=` drops it)
      class_tie           ncls >= 5: a prior's best score is held by two classes (the cross-class rule labels it with the lower)
      over_top_k          top_k 10 and more than 10 priors pass the pre-filter in one class
      over_trad_cap       trad_cap 64 and one class holds more than 64 candidates (P >= 65)
      P_below_wave        P < 64"""
    from oracle import ora
    assert profile in YOLACT_PROFILES
    rng = _rng("yolact_detect", profile, seed)
    N, P, ncls = int(rng.integers(1, 4)), int(rng.integers(1, 401)), int(rng.choice([2, 5, 81]))
    trad_cap, top_k, max_det = int(rng.choice([64, 128])), int(rng.choice([10, 200])), int(rng.choice([5, 100]))
    if profile == "empty_next_to_full":
        N, P = max(N, 2), max(P, 4)
    elif profile in ("identical_boxes", "class_tie"):
        P = max(P, 2)
    elif profile == "iou_at_threshold":
        P = max(P, 4)
    elif profile == "over_top_k":
        top_k, P = 10, max(P, 12)
    elif profile == "over_trad_cap":
        trad_cap, P = 64, int(rng.integers(66, 401))
    elif profile == "P_below_wave":
        P = int(rng.integers(1, 64))
    if profile == "class_tie":
        ncls = int(rng.choice([5, 81]))
    x, y = rng.integers(0, 48, P) * 8.0, rng.integers(0, 48, P) * 8.0
    wh = rng.integers(1, 9, (P, 2)) * 8.0
    px = np.stack([x, y, x + wh[:, 0], y + wh[:, 1]], 1)
    conf = np.full((N, P, ncls), -12.0, F)
    conf[..., 0] = 0.0
    hot = rng.uniform(0, 1, (N, P)) < 0.5
    few = 1 + rng.integers(0, min(ncls - 1, 3), (N, P, 2))                     # a few classes collect the candidates
    for n in range(N):
        idx = np.flatnonzero(hot[n])
        conf[n, idx, few[n, idx, 0]] = _q(rng, -2, 6, len(idx))
        two = idx[rng.uniform(0, 1, len(idx)) < 0.3]
        conf[n, two, few[n, two, 1]] = _q(rng, -2, 6, len(two))
    pair = None
    if profile == "empty_next_to_full":
        conf[0, :, 0] = 30.0
        conf[1, :, 1] = _q(rng, 0, 6, P)
    elif profile == "identical_boxes":
        px[:] = px[0]
        conf[0, :, 1] = _q(rng, 0, 6, P)
    elif profile == "iou_at_threshold":
        ox, oy = float(rng.integers(0, 40)) * 8.0, float(rng.integers(0, 40)) * 8.0
        pair = rng.choice(P, 4, replace=False)
        px[pair] = np.array([[0, 0, 16, 16], [0, 0, 16, 8], [64, 64, 67, 67], [64, 64, 67, 65]], np.float64) + [ox, oy, ox, oy]
        conf[0, pair, 1:] = -12.0
        conf[0, pair, 1] = (7.0, 6.75, 6.5, 6.25)
    elif profile == "class_tie":
        p0 = int(rng.integers(0, P))
        a, b = np.sort(rng.choice(np.arange(1, ncls), 2, replace=False))
        conf[0, p0, 1:] = -12.0
        conf[0, p0, [a, b]] = 3.0
    elif profile in ("over_top_k", "over_trad_cap"):
        conf[0, :, 1] = _q(rng, 0, 6, P)
    priors = _px_priors(px)
    loc = np.zeros((N, P, 4), F)
    mask = np.tanh(rng.standard_normal((N, P, 4))).astype(F)
    par = dict(conf_thresh=0.05, nms_thr=0.5, top_k=top_k, max_det=max_det, max_size=YOLACT_MAX_SIZE, cap=trad_cap)
    prob = [ora.softmax(conf[n]) for n in range(N)]
    boxes = ora.yolact_decode(loc[0], priors)
    passing = [(p[:, 1:].max(1) > F(0.05)) for p in prob]
    reached = set()
    if any(not passing[n].any() and passing[n + 1].sum() >= 2 for n in range(N - 1)):
        reached.add("empty_next_to_full")
    if P >= 2 and (boxes == boxes[0]).all() and passing[0].sum() >= 2:
        reached.add("identical_boxes")
    if pair is not None and passing[0][pair].all():
        import yolact_nms_ref
        j = yolact_nms_ref.jaccard(boxes[pair[:2]])[0, 1]
        kept = yolact_nms_ref.cnms_keep(boxes[pair[2:]] * F(YOLACT_MAX_SIZE), 0.5), yolact_nms_ref.cnms_keep(boxes[pair[2:]] * F(YOLACT_MAX_SIZE), np.nextafter(F(0.5), F(1)))
        if j == F(0.5) and len(kept[0]) == 1 and len(kept[1]) == 2:
            reached.add("iou_at_threshold")
    fg = prob[0][:, 1:]
    if ncls >= 3 and (passing[0] & ((fg == fg.max(1, keepdims=True)).sum(1) >= 2)).any():
        reached.add("class_tie")
    if passing[0].sum() > top_k:
        reached.add("over_top_k")
    if ((fg > F(0.05)).sum(0) > trad_cap).any():
        reached.add("over_trad_cap")
    if P < 64:
        reached.add("P_below_wave")
    return dict(op="yolact_detect", profile=profile, seed=seed, conf=conf, loc=loc, mask=mask, priors=priors, params=par, reached=reached)


def ref_yolact_detect(case, modes=(0, 1, 2)):
    """-> {mode: [(detections, nms_total or None, overflow) per image]}"""
    import yolact_nms_ref
    from oracle import ora
    p = case["params"]
    out = {}
    for mode in modes:
        rows = []
        for n in range(case["conf"].shape[0]):
            prob, boxes = ora.softmax(case["conf"][n]), ora.yolact_decode(case["loc"][n], case["priors"])
            if mode == 0:
                rows.append((ora.yolact_detect(prob, boxes, case["mask"][n], p["conf_thresh"], p["nms_thr"], p["top_k"], p["max_det"]), None, 0))
            else:
                rows.append(yolact_nms_ref.run_ref(mode, prob, boxes, case["mask"][n], p["conf_thresh"], p["nms_thr"], p["top_k"], p["max_det"], p["max_size"], p["cap"]))
        out[mode] = rows
    return out


# ============================================================================================================ bbox_aug_candidates over views, then the merge
BBOX_AUG_PROFILES = ("pool_overflow_mid_row", "zero_proposals", "flip_and_ratio", "at_threshold", "agnostic")
_threshold_rows = {}


def _on_threshold_row(ncls, cls):
    """a logit row whose probability of class `cls` is exactly 0.05f under the oracle's softmax (tests/decision_cases.threshold_logits; searched once)"""
    if (ncls, cls) not in _threshold_rows:
        from decision_cases import threshold_logits
        from oracle import ora
        _threshold_rows[(ncls, cls)] = threshold_logits(ora.softmax, 0.05, ncls, cls=cls)["on"]
    return _threshold_rows[(ncls, cls)]


def build_bbox_aug(profile, seed):
    """1..3 views of N 1..3 images with R 1..70 proposals a view, ncls in {2, 5, 81}, a pool of cap in {1, 64, 8192}; thr 0.05.  Logits are multiples of 1/4
    (background 0, foreground in [-6, 1]); proposals are integer boxes on a 10-pixel grid inside their view; view 0 has zero regressions, the others random
    ones; prop_cnt is random and the rows past it hold NaN.  The merge runs class-wise NMS over the pool with random nms_flags and det_per_img in {3, 100}.
      pool_overflow_mid_row  ncls >= 5, cap 1 or 64, view 0 of image 0: every proposal passes in exactly three classes and there are enough of them
                             (R >= 22) to overflow the pool: the cap falls inside a proposal's run of classes (1 and 64 are no multiples of 3)
      zero_proposals         an image without proposals in view 0 (N >= 2) next to one that has candidates
      flip_and_ratio         two views or more; the last is mirrored and smaller than view 0 (ratios != 1) and holds a candidate of image 0
      at_threshold           ncls >= 5: a proposal's class probability is exactly 0.05f, which `>` rejects
      agnostic               class-agnostic regression ([N, R, 8])"""
    import bbox_aug_ref
    from oracle import ora
    assert profile in BBOX_AUG_PROFILES
    rng = _rng("bbox_aug", profile, seed)
    nv, N, R = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 71))
    ncls, cap = int(rng.choice([2, 5, 81])), int(rng.choice([1, 64, 8192]))
    agnostic = bool(rng.integers(0, 2)) or profile == "agnostic"
    if profile == "pool_overflow_mid_row":
        ncls, cap, R = int(rng.choice([5, 81])), int(rng.choice([1, 64])), int(rng.integers(22, 71))
    elif profile == "zero_proposals":
        N = max(N, 2)
    elif profile == "flip_and_ratio":
        nv = max(nv, 2)
    elif profile == "at_threshold":
        ncls = int(rng.choice([5, 81]))
    hw0 = (300, 400)
    views = []
    for v in range(nv):
        hw = hw0 if v == 0 else (int(rng.integers(12, 31)) * 10, int(rng.integers(16, 41)) * 10)
        if profile == "flip_and_ratio" and v == nv - 1:
            hw = (200, 300)
        logits = np.concatenate([np.zeros((N, R, 1), F), _q(rng, -6, 1, (N, R, ncls - 1))], -1)
        x = rng.integers(0, (hw[1] - 50) // 10, (N, R)) * 10.0; y = rng.integers(0, (hw[0] - 50) // 10, (N, R)) * 10.0
        wh = rng.integers(1, 6, (N, R, 2)) * 10.0
        props = np.stack([x, y, x + wh[..., 0] - 1, y + wh[..., 1] - 1], -1).astype(F)
        regr = np.zeros((N, R, 8 if agnostic else 4 * ncls), F) if v == 0 else rng.normal(0, 0.3, (N, R, 8 if agnostic else 4 * ncls)).astype(F)
        cnt = rng.integers(0, R + 1, N).astype(np.int32)
        cnt[0] = max(cnt[0], 1)
        hflip = bool(rng.integers(0, 2)) or (profile == "flip_and_ratio" and v == nv - 1)
        views.append(dict(logits=logits, regr=regr, props=props, cnt=cnt, hw=np.tile(np.array(hw, np.int32), (N, 1)), hflip=hflip,
                          ratios=np.array(bbox_aug_ref.view_ratios(hw0, hw), F)))
    v0 = views[0]
    if profile == "pool_overflow_mid_row":
        v0["cnt"][0] = R
        v0["logits"][0, :, 1:] = -20.0
        for r in range(R):
            v0["logits"][0, r, rng.choice(np.arange(1, ncls), 3, replace=False)] = 0.0        # three classes at 1/4 each
    elif profile == "zero_proposals":
        v0["cnt"][0], v0["cnt"][1] = 0, max(v0["cnt"][1], 1)
        v0["logits"][1, 0, 1] = 1.0
    elif profile == "at_threshold":
        v0["logits"][0, 0] = _on_threshold_row(ncls, int(rng.integers(1, ncls)))
    elif profile == "flip_and_ratio":
        views[-1]["logits"][0, 0, 1] = 1.0                     # the mirrored view has a candidate
    for v in views:
        for n in range(N):
            for k in ("logits", "regr", "props"):
                v[k][n, v["cnt"][n]:] = np.nan
    post = dict(nms_thr=0.5, det_per_img=int(rng.choice([3, 100])), cap=100, nms_flags=int(rng.integers(0, 8)))
    case = dict(op="bbox_aug", profile=profile, seed=seed, views=views, ncls=ncls, cap=cap, thr=0.05, agnostic=agnostic, post=post)
    reached = set()
    p0 = ora.softmax(v0["logits"][0, :v0["cnt"][0]]) if v0["cnt"][0] else np.zeros((0, ncls), F)
    ok = p0 > F(0.05)
    ok[:, 0] = False
    rows = np.nonzero(ok)[0]
    if len(rows) > cap and rows[cap - 1] == rows[cap]:
        reached.add("pool_overflow_mid_row")
    if any(v0["cnt"][n] == 0 and v0["cnt"][n + 1] > 0 for n in range(N - 1)) and len(ref_bbox_aug(case)["pools"][1][0][1]):
        reached.add("zero_proposals")
    vl = views[-1]
    if nv >= 2 and vl["hflip"] and (vl["ratios"] != 1).all() and len(bbox_aug_ref.candidates(vl["logits"][0], vl["regr"][0], vl["props"][0], vl["cnt"][0], vl["hw"][0], True, vl["ratios"],
                                                                                             0.05, agnostic)[1]):
        reached.add("flip_and_ratio")
    if (p0[:, 1:] == F(0.05)).any():
        reached.add("at_threshold")
    if agnostic:
        reached.add("agnostic")
    return dict(case, reached=reached)


def ref_bbox_aug(case, wrong=None):
    """-> pools[n] = ((boxes, scores, labels) of the capped pool, total), dets[n] = the merge over it"""
    import bbox_aug_ref as br
    pools, dets = [], []
    for n in range(case["views"][0]["logits"].shape[0]):
        cands = [br.candidates(v["logits"][n], v["regr"][n], v["props"][n], v["cnt"][n], v["hw"][n], v["hflip"], v["ratios"], case["thr"], case["agnostic"], wrong)
                 for v in case["views"]]
        pooled, total = br.pool(cands, case["cap"])
        pools.append((pooled, total))
        dets.append(br.merge(pooled, case["ncls"], **case["post"]))
    return dict(pools=pools, dets=dets)


OPS.update({
    "yolact_detect": (build_yolact_detect, ref_yolact_detect, YOLACT_PROFILES),
    "bbox_aug": (build_bbox_aug, ref_bbox_aug, BBOX_AUG_PROFILES),
})
