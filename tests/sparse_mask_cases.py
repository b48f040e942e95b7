"""Inputs, reference windows and checkers of the sparse-mask contract between the two mask writers (paste_masks_kernel, yolact_upsample_masks_kernel)
and the run-length encoder that reads their planes through the windows they report.  numpy only: the oracle and the device are handed in.

The contract, per slot below its image's count:
  containment  every set pixel of the dense oracle plane lies inside the reported window;
  coverage     every byte inside the window equals the dense oracle plane (the encoder reads all of them, and the plane held something else before);
  confinement  nothing outside the window changes -- but for the paste's whole-word store, which may put a 0 into the at most three bytes that share a
               4-byte word with an end of a window row segment (the encoder of this slot does not read them; no other slot's bytes are in reach).
Slots past the count: neither their plane nor their window entry is written.

The checkers take what a writer left (`planes`, `wins`), what was there before the launch (`before`, `wins_before`) and the dense oracle planes; the CPU
tests run them on numpy models of the two writers (and on mutated models, to show that each checker can fail), the GPU tests on the device's output."""
import numpy as np

F32 = np.float32
POISON = 0xA5          # every output byte before a first launch: neither 0 nor 1
WIN_POISON = -1        # every window entry before a first launch (an (x0, y0, x1, y1) of -1 is no window a writer emits for a live slot)
N_IMAGES = 3

# ------------------------------------------------------------------------------------------------------------------ paste (Masker) inputs
# 13 rows x 16..19 columns: every im_w % 4 (where a row's first word starts relative to the window); widths 1 and 2: a 4-byte word reaches two rows
# away; 130 x 21 and 200 x 150: windows that start beyond the encoder's 64-row chunk 0 and end exactly on rows 64, 128 and 192
PASTE_PLANES = [(13, 16), (13, 17), (13, 18), (13, 19), (7, 1), (5, 2), (130, 21), (200, 150)]
PASTE_M = [28, 14]
# slots whose dense plane has a set pixel on the first and the last row and column of the reference window (an all-ones mask; the window is either
# clipped by the image on that side, or at most 5 pixels long, so that with M = 14 its end pixels sample the mask and not the zero padding)
PASTE_BORDER = ("small_interior", "touch_left", "touch_top", "touch_right", "touch_bottom", "over_all", "bottom_inner", "bottom_edge", "narrow_all")
# slots whose window touches the last row with its last column set there: a run that closes in row 0 of column x1 (x1 < w), or at h * w (x1 == w)
PASTE_BOTTOM_INNER = ("bottom_inner", "bottom_from_chunk1")
PASTE_BOTTOM_EDGE = ("bottom_edge",)
PASTE_EMPTY = ("out_left", "out_right", "out_top", "out_bottom", "out_top_left", "out_bottom_right")
PASTE_BOTH_NEGATIVE = ("out_top_left", "out_bottom_right")   # x1 < x0 and y1 < y0: the kernel's item count is a product of two negatives


def masker_window(boxes, M, im_h, im_w):
    """Masker(padding = 1)'s paste window restated in fp32: expand the box about its centre by (M + 2) / M, truncate the corners to int, + 1 on the far
    corner, clamp to the image -> int64 [..., 4] (x0, y0, x1, y1); x1 <= x0 or y1 <= y0: nothing is pasted."""
    b = np.asarray(boxes, F32)
    scale = F32(M + 2) / F32(M)
    out = np.zeros(b.shape, np.int64)
    for ax, size in ((0, im_w), (1, im_h)):
        lo, hi = b[..., ax], b[..., ax + 2]
        half = ((hi - lo) * F32(0.5)) * scale
        c = (hi + lo) * F32(0.5)
        p1 = np.trunc(c - half).astype(np.int64)
        p2 = np.trunc(c + half).astype(np.int64)
        out[..., ax] = np.maximum(p1, 0)
        out[..., ax + 2] = np.minimum(p2 + 1, size)
    return out


def box_for_window(ux0, uy0, ux1, uy1, M):
    """a box whose expanded corners truncate to the unclamped window [ux0, ux1) x [uy0, uy1): each expanded corner sits half a pixel inside the
    integer it truncates to (truncation is toward zero: below zero that is half a pixel further out)"""
    out = np.zeros(4, np.float64)
    for ax, (p1, p2) in enumerate(((ux0, ux1 - 1), (uy0, uy1 - 1))):
        lo = p1 + 0.5 if p1 >= 0 else p1 - 0.5
        hi = p2 + 0.5 if p2 >= 0 else p2 - 0.5
        c, half = (lo + hi) / 2, (hi - lo) / 2 * M / (M + 2)
        out[ax], out[ax + 2] = c - half, c + half
    return out.astype(F32)


def paste_boxes(h, w, M):
    """[(name, box, unclamped window or None)] for an h x w plane: all finite"""
    def W(name, *u):
        return (name, box_for_window(*u, M), u)

    def raw(name, *b):
        return (name, np.array(b, F32), None)
    if w < 3:     # the narrow planes: every window is as wide as the image or empty
        return [raw("full", 0, 0, w - 1, h - 1), W("narrow_all", -3, -3, w + 3, h + 3), W("narrow_rows", 0, 1, w, 3), W("narrow_col0", 0, 2, 1, h),
                W("narrow_last", w - 1, h - 2, w, h + 2), W("out_left", -40, 1, -20, h - 1), W("out_bottom_right", w + 25, h + 31, w + 60, h + 75),
                raw("one_pixel", 0, 2, 0, 2), raw("reversed", w - 1, h - 1, 0, 0)]
    s = 4
    out = [
        W("small_interior", 5, 4, 5 + s, 4 + s),
        W("touch_left", 0, 4, s, 4 + s), W("touch_top", 6, 0, 6 + s, s), W("touch_right", w - s, 4, w, 4 + s), W("touch_bottom", 3, h - s, 3 + s, h),
        W("over_left", -3, 4, 3, 9), W("over_top", 6, -3, 11, 3), W("over_right", w - 3, 4, w + 3, 9),
        W("bottom_inner", 3, h - 3, 3 + s, h + 4),        # overhangs the last row, x1 < w
        W("bottom_edge", w - 3, h - 3, w + 4, h + 4),     # overhangs the last row and the last column: x1 == w
        W("over_all", -(w // 4 + 6), -(h // 4 + 6), w + w // 4 + 6, h + h // 4 + 6),   # far enough out that the mask's zero padding stays outside the image
        raw("full", 0, 0, w - 1, h - 1),
        W("out_left", -40, 2, -20, h - 2), W("out_right", w + 20, 2, w + 40, h - 2), W("out_top", 2, -40, w - 2, -20), W("out_bottom", 2, h + 20, w - 2, h + 40),
        W("out_top_left", -40, -50, -20, -30), W("out_bottom_right", w + 25, h + 31, w + 60, h + 75),
        raw("one_pixel", 5, 6, 5, 6),
        raw("reversed", w * 0.8, h * 0.7, w * 0.2, h * 0.1),
        raw("fractional", 0.3, 0.2, w * 0.7 + 0.4, h * 0.6 + 0.3),
        W("wide_interior", 2, 1, w - 1, h - 2),
    ]
    if h >= 130:
        out += [W("chunk1_to_128", 5, 70, 9, 128), W("ends_on_64", 2, 3, 12, 64), W("one_row_64", 7, 64, 15, 65),
                W("bottom_from_chunk1", 5, 100, 9, h + 10)]     # touches the last row from a window that starts beyond chunk 0
    if h >= 200:
        out += [W("ends_on_192", 100, 130, 140, 192), W("chunk1_only", 20, 64, 24, 128)]
    return out


def step_counts(K, step):
    """0, 1, K - 1 and K over the three images of the two steps"""
    return np.array([[K, K - 1, 0], [1, 0, K]][step], np.int32)


def _slot_order(K, n, step):
    """which box of the list slot k of image n holds: another one in every image, and another one again in the second step"""
    order = np.roll(np.arange(K), -(5 * n + 7 * step))
    return order[::-1] if step else order


def paste_case(h, w, M, step=0):
    """-> dict(h, w, M, names [N][K], boxes [N,K,4], masks [N,K,M,M], counts [N], unclamped [N][K])"""
    rng = np.random.default_rng(100000 * step + 1000 * h + 10 * w + M)
    lst = paste_boxes(h, w, M)
    K = len(lst)
    solid = set(PASTE_BORDER + PASTE_BOTTOM_INNER + PASTE_BOTTOM_EDGE)
    names, boxes, unclamped = [], np.zeros((N_IMAGES, K, 4), F32), []
    masks = rng.uniform(0.25, 1.0, (N_IMAGES, K, M, M)).astype(F32)      # a noisy blend around thr: many short runs
    for n in range(N_IMAGES):
        order = _slot_order(K, n, step)
        names.append([lst[i][0] for i in order]); unclamped.append([lst[i][2] for i in order])
        for k, i in enumerate(order):
            boxes[n, k] = lst[i][1]
            if lst[i][0] in solid:
                masks[n, k] = 1.0
    return dict(h=h, w=w, M=M, names=names, boxes=boxes, masks=masks, counts=step_counts(K, step), unclamped=unclamped)


def paste_dense(ora, case):
    """the dense oracle planes [N, K, h, w]; zero past the count"""
    N, K = case["boxes"].shape[:2]
    out = np.zeros((N, K, case["h"], case["w"]), np.uint8)
    for n in range(N):
        c = int(case["counts"][n])
        if c:
            out[n, :c] = ora.paste_masks(case["masks"][n, :c], case["boxes"][n, :c], case["h"], case["w"], 0.5)
    return out


# ------------------------------------------------------------------------------------------------------------------ Yolact inputs
# (PH, PW, h, w, image_hw or None): prototype maps of 9 x 8 and 23 x 31 under planes below, equal to and above them; the ragged launches put all three
# relations into one common plane
YOLACT_SHAPES = [
    (9, 8, 13, 19, ((13, 19), (9, 8), (5, 6))),
    (9, 8, 9, 8, None),
    (9, 8, 5, 6, None),
    (9, 8, 13, 16, None),
    (23, 31, 200, 150, ((200, 150), (23, 31), (64, 17))),
    (23, 31, 23, 31, None),
    (23, 31, 130, 21, None),
]
YOLACT_K = 27   # more than one group of 25 detections of the prototype stage
YOLACT_BOXES = [
    ("interior", (0.3, 0.25, 0.7, 0.8)),
    ("touch_left", (0.0, 0.2, 0.4, 0.6)), ("touch_top", (0.5, 0.0, 0.9, 0.5)), ("touch_right", (0.6, 0.3, 1.0, 0.7)), ("touch_bottom", (0.2, 0.5, 0.6, 1.0)),
    ("over_left", (-0.2, 0.3, 0.3, 0.7)), ("over_top", (0.3, -0.3, 0.7, 0.4)), ("over_right", (0.6, 0.2, 1.3, 0.6)), ("over_bottom", (0.2, 0.6, 0.5, 1.4)),
    ("bottom_edge", (0.6, 0.6, 1.2, 1.3)),                      # reaches the last row and the last column: x1 == w
    ("out_left", (-0.9, 0.2, -0.5, 0.8)), ("out_right", (1.5, 0.2, 1.9, 0.8)), ("out_top", (0.2, -0.9, 0.8, -0.5)), ("out_bottom", (0.2, 1.5, 0.8, 1.9)),
    ("out_top_left", (-0.9, -0.8, -0.5, -0.4)), ("out_bottom_right", (1.4, 1.5, 1.8, 1.9)),
    ("one_pixel", (0.5, 0.5, 0.5, 0.5)),
    ("reversed", (0.8, 0.7, 0.2, 0.1)),
    ("full", (0.0, 0.0, 1.0, 1.0)),
    ("over_all", (-0.5, -0.5, 1.5, 1.5)),
    ("near_left", (-0.3, 0.1, -0.01, 0.9)),                      # outside by a hair: the 1-pixel padding brings proto column 0 back in
    ("near_bottom", (0.1, 1.01, 0.9, 1.2)),
]
YOLACT_EMPTY = ("out_left", "out_right", "out_top", "out_bottom", "out_top_left", "out_bottom_right")
YOLACT_SOLID = ("interior", "touch_left", "touch_top", "touch_right", "touch_bottom", "over_left", "over_top", "over_right", "over_bottom", "bottom_edge",
                "full", "over_all", "one_pixel")
YOLACT_BOTTOM = ("over_bottom", "touch_bottom")   # reach the last row with x1 < w
YOLACT_BOTTOM_EDGE = ("bottom_edge", "full", "over_all")


def yolact_case(PH, PW, h, w, image_hw, step=0):
    """-> dict(PH, PW, h, w, image_hw [N,2] or None, names [N][K], proto [N,PH,PW,32], coeffs [N,K,32], boxes [N,K,4] relative, counts [N])"""
    rng = np.random.default_rng(100000 * step + 1000 * PH + 10 * h + w)
    K = YOLACT_K
    lst = list(YOLACT_BOXES)
    while len(lst) < K:       # filled up with random finite boxes, some of them overhanging
        c, s = rng.uniform(0.0, 1.0, 2), rng.uniform(0.05, 0.8, 2)
        lst.append(("random%d" % len(lst), tuple(np.concatenate([c - s / 2, c + s / 2]))))
    proto = np.abs(rng.standard_normal((N_IMAGES, PH, PW, 32))).astype(F32)
    coeffs = rng.standard_normal((N_IMAGES, K, 32)).astype(F32)
    boxes = np.zeros((N_IMAGES, K, 4), F32)
    names = []
    for n in range(N_IMAGES):
        order = _slot_order(K, n, step)
        names.append([lst[i][0] for i in order])
        for k, i in enumerate(order):
            boxes[n, k] = lst[i][1]
            if lst[i][0] in YOLACT_SOLID:
                coeffs[n, k] = np.abs(coeffs[n, k]) * F32(0.5)          # a positive logit everywhere: the mask fills its crop up to the edge
    ihw = None if image_hw is None else np.array(image_hw, np.int32).reshape(N_IMAGES, 2)
    return dict(PH=PH, PW=PW, h=h, w=w, image_hw=ihw, names=names, proto=proto, coeffs=coeffs, boxes=boxes, counts=step_counts(K, step))


def image_sizes(case):
    """[N][2] (h_n, w_n): the part of the common plane image n occupies"""
    N = case["boxes"].shape[0]
    return np.tile(np.array([[case["h"], case["w"]]], np.int32), (N, 1)) if case.get("image_hw") is None else case["image_hw"]


def yolact_dense(ora, case):
    """the dense oracle planes [N, K, h, w] (image n assembled at its own size in the top-left corner; zero elsewhere and past the count) and the
    prototype-resolution masks [N, K, PH, PW] (zero past the count)"""
    N, K = case["boxes"].shape[:2]
    out = np.zeros((N, K, case["h"], case["w"]), np.uint8)
    lo = np.zeros((N, K, case["PH"], case["PW"]), F32)
    hw = image_sizes(case)
    for n in range(N):
        c = int(case["counts"][n])
        if c:
            hn, wn = int(hw[n, 0]), int(hw[n, 1])
            out[n, :c, :hn, :wn] = ora.yolact_masks(case["proto"][n], case["coeffs"][n, :c], case["boxes"][n, :c], hn, wn)[0]
            lo[n, :c] = ora.yolact_proto_masks(case["proto"][n], case["coeffs"][n, :c], case["boxes"][n, :c])
    return out, lo


def yolact_crop(box, PH, PW):
    """sanitize_coordinates(padding = 1, cast = False) in fp32 -> (x1, x2, y1, y2): prototype pixel i is inside when x1 <= i < x2"""
    out = []
    for ax, size in ((0, PW), (1, PH)):
        a, b = F32(box[ax]) * F32(size), F32(box[ax + 2]) * F32(size)
        lo, hi = (a, b) if a < b else (b, a)
        lo, hi = F32(lo - F32(1.0)), F32(hi + F32(1.0))
        out += [lo if lo > 0 else F32(0.0), hi if hi < F32(size) else F32(size)]
    return tuple(out)


def bilinear_taps(in_sz, out_sz):
    """the two source indices of every destination pixel of an align_corners = False resize, in fp32 as the oracle's bil_coef computes them"""
    scale = F32(in_sz) / F32(out_sz)
    src = scale * (np.arange(out_sz, dtype=F32) + F32(0.5)) - F32(0.5)
    src = np.maximum(src, F32(0.0))
    i0 = np.minimum(src.astype(np.int64), in_sz - 1)
    return i0, np.minimum(i0 + 1, in_sz - 1)


def yolact_tap_bounds(box, PH, PW, h, w):
    """per axis the bounding interval [lo, hi) of the output pixels one of whose two taps lies in the sanitized crop, or None when there is none:
    -> ((x_lo, x_hi) or None, (y_lo, y_hi) or None).  A pixel outside either interval blends four zeros."""
    x1, x2, y1, y2 = yolact_crop(box, PH, PW)
    out = []
    for lo, hi, in_sz, out_sz in ((x1, x2, PW, w), (y1, y2, PH, h)):
        i0, i1 = bilinear_taps(in_sz, out_sz)
        ok = ((i0.astype(F32) >= lo) & (i0.astype(F32) < hi)) | ((i1.astype(F32) >= lo) & (i1.astype(F32) < hi))
        idx = np.nonzero(ok)[0]
        out.append(None if idx.size == 0 else (int(idx[0]), int(idx[-1]) + 1))
    return tuple(out)


YOLACT_MARGIN = 3   # the kernel's stated 2 pixels of slack + 1 for the float rounding of the bound


def check_yolact_window_bounds(case, wins):
    """the conservative window of every live slot holds the tap set's bounding box and stays within YOLACT_MARGIN pixels of it on every side.  On an
    axis without any such pixel the slot's plane is all zero and there is no box to grow; the crop then holds no prototype pixel that an output pixel
    taps, so what the kernel bounds is the footprint of at most one prototype pixel, out / in output pixels (under a reduction: less than one),
    and the window may be that long plus the margin on both sides -- still far from the whole plane on every shape but the smallest."""
    hw = image_sizes(case)
    for n in range(case["boxes"].shape[0]):
        for k in range(int(case["counts"][n])):
            bx, by = yolact_tap_bounds(case["boxes"][n, k], case["PH"], case["PW"], int(hw[n, 0]), int(hw[n, 1]))
            x0, y0, x1, y1 = (int(v) for v in wins[n, k])
            where = (n, k, case["names"][n][k], (x0, y0, x1, y1), bx, by)
            assert 0 <= x0 and 0 <= y0 and x1 <= int(hw[n, 1]) and y1 <= int(hw[n, 0]), ("window leaves the image",) + where
            for (a0, a1), b, fs in (((x0, x1), bx, int(hw[n, 1]) / case["PW"]), ((y0, y1), by, int(hw[n, 0]) / case["PH"])):
                if b is None:
                    assert a1 - a0 <= 2 * YOLACT_MARGIN + int(np.ceil(max(fs, 1.0))), ("window on an axis without a live tap",) + where
                else:
                    assert a0 <= b[0] and a1 >= b[1], ("window misses a pixel with a live tap",) + where
                    assert a0 >= b[0] - YOLACT_MARGIN and a1 <= b[1] + YOLACT_MARGIN, ("window wider than the tap set + margin",) + where


# ------------------------------------------------------------------------------------------------------------------ the contract checkers
def window_mask(win, h, w):
    """bool [h, w]: the pixels inside (x0, y0, x1, y1) clamped to the plane"""
    x0, y0, x1, y1 = (int(v) for v in win)
    m = np.zeros((h, w), bool)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    if x1 > x0 and y1 > y0:
        m[y0:y1, x0:x1] = True
    return m


def paste_spill_mask(win, h, w):
    """bool [h, w]: the bytes outside the window within 3 bytes, in flat order, of an end of one of its row segments (where the paste's whole-word
    store may leave a 0)"""
    inside = window_mask(win, h, w).reshape(-1)
    near = inside.copy()
    for d in (1, 2, 3):
        near[d:] |= inside[:-d]
        near[:-d] |= inside[d:]
    return (near & ~inside).reshape(h, w)


def check_containment(dense, wins, counts, names):
    N, K, h, w = dense.shape
    for n in range(N):
        for k in range(int(counts[n])):
            stray = dense[n, k].astype(bool) & ~window_mask(wins[n, k], h, w)
            assert not stray.any(), ("set pixel outside the reported window", n, k, names[n][k], tuple(wins[n, k]), np.argwhere(stray)[:4].tolist())


def check_coverage(planes, dense, wins, counts, names):
    N, K, h, w = dense.shape
    for n in range(N):
        for k in range(int(counts[n])):
            m = window_mask(wins[n, k], h, w)
            bad = m & (planes[n, k] != dense[n, k])
            assert not bad.any(), ("byte inside the window differs from the dense plane", n, k, names[n][k], tuple(wins[n, k]), np.argwhere(bad)[:4].tolist(),
                                   planes[n, k][bad][:4].tolist())


def check_confinement(planes, before, wins, counts, names, spill):
    """outside its window a live slot's plane is what it was before the launch; spill = True admits a 0 in paste_spill_mask"""
    N, K, h, w = planes.shape
    for n in range(N):
        for k in range(int(counts[n])):
            out = ~window_mask(wins[n, k], h, w)
            changed = out & (planes[n, k] != before[n, k])
            if spill:
                changed &= ~(paste_spill_mask(wins[n, k], h, w) & (planes[n, k] == 0))
            assert not changed.any(), ("byte outside the window was written", n, k, names[n][k], tuple(wins[n, k]), np.argwhere(changed)[:4].tolist())


def check_dead_slots(planes, before, wins, wins_before, counts):
    for n in range(planes.shape[0]):
        c = int(counts[n])
        assert np.array_equal(planes[n, c:], before[n, c:]), ("plane of a slot past the count was written", n)
        assert np.array_equal(wins[n, c:], wins_before[n, c:]), ("window of a slot past the count was written", n)


def check_dense_equals_sparse(cleared, sparse, wins, counts):
    """the clear = 1 planes: the sparse planes inside the windows, 0 everywhere else (slots past the count included)"""
    N, K, h, w = cleared.shape
    for n in range(N):
        for k in range(K):
            m = window_mask(wins[n, k], h, w) if k < int(counts[n]) else np.zeros((h, w), bool)
            assert np.array_equal(cleared[n, k][m], sparse[n, k][m]) and not cleared[n, k][~m].any(), (n, k)


def check_chain(encode, ora, planes, counts, wins, dense, image_hw=None):
    """encode(planes, counts, image_hw, windows) -> (run_off, counts, str_off, chars, status) as isegmi's rle_encode returns them: the counts and the
    string of every live slot are those of the dense oracle plane (cropped to the image's own size), dead slots own nothing"""
    N, K, h, w = planes.shape
    ro, cn, so, ch, st = encode(planes, counts, image_hw, wins)
    assert st[2] == 0, "overflow flagged"
    for n in range(N):
        hi, wi = (h, w) if image_hw is None else (int(image_hw[n][0]), int(image_hw[n][1]))
        for k in range(K):
            m = n * K + k
            if k >= int(counts[n]):
                assert ro[m + 1] == ro[m] and so[m + 1] == so[m], (n, k)
                continue
            ref = ora.rle_encode(dense[n, k, :hi, :wi])
            got = np.asarray(cn[ro[m]:ro[m + 1]])
            assert np.array_equal(got, ref), ("run counts through the window", n, k, tuple(wins[n, k]), got[:8].tolist(), ref[:8].tolist())
            assert bytes(ch[so[m]:so[m + 1]]).decode("ascii") == ora.rle_to_string(ref), ("string through the window", n, k)


def windowed_encoder(ora):
    """the numpy model of the device encoder: a plane is read through its window alone -- everything outside it counts as zero -- and the result has
    the layout of isegmi's rle_encode"""
    def encode(planes, counts, image_hw, wins):
        N, K, h, w = planes.shape
        ro, so, cn, ch = [0], [0], [], b""
        for n in range(N):
            hi, wi = (h, w) if image_hw is None else (int(image_hw[n][0]), int(image_hw[n][1]))
            for k in range(K):
                if k < int(counts[n]):
                    seen = np.where(window_mask(wins[n, k], h, w), planes[n, k], 0)[:hi, :wi] if wins is not None else planes[n, k, :hi, :wi]
                    c = ora.rle_encode(seen != 0)
                    cn.append(c); ch += ora.rle_to_string(c).encode("ascii")
                ro.append(sum(len(c) for c in cn)); so.append(len(ch))
        return np.array(ro), (np.concatenate(cn) if cn else np.zeros(0, np.uint32)), np.array(so), ch, np.array([ro[-1], so[-1], 0, 0])
    return encode


# ------------------------------------------------------------------------------------------------------------------ numpy models of the two writers
def model_paste(case, dense, planes, wins, mutate=None):
    """what paste_masks_kernel leaves with clear = 0: per live slot the reference window, and per window row the 4-byte words (aligned to the plane's
    first byte) that overlap the row's segment, stored whole -- dense values inside the window, zeros in the rest of the word.
    mutate: 'window_short_column' (reports x1 - 1), 'skip_last_word' (a row's last word is not stored), 'clear_rows' (zeroes the window's rows at
    full width), 'write_dead' (also writes the first slot past the count)"""
    planes, wins = planes.copy(), wins.copy()
    N, K, h, w = planes.shape
    ref = masker_window(case["boxes"], case["M"], h, w)
    for n in range(N):
        live = int(case["counts"][n]) + (1 if mutate == "write_dead" else 0)
        for k in range(min(live, K)):
            x0, y0, x1, y1 = (int(v) for v in ref[n, k])
            wins[n, k] = (x0, y0, x1 - 1 if mutate == "window_short_column" else x1, y1)
            if x1 <= x0 or y1 <= y0:
                continue
            flat, src, inside = planes[n, k].reshape(-1), dense[n, k].reshape(-1), window_mask(ref[n, k], h, w).reshape(-1)
            for y in range(y0, y1):
                beg, end = y * w + x0, y * w + x1
                words = list(range(beg & ~3, end, 4))
                if mutate == "skip_last_word":
                    words = words[:-1]
                for q in words:
                    for f in range(q, min(q + 4, h * w)):
                        flat[f] = src[f] if inside[f] else 0
                if mutate == "clear_rows":
                    planes[n, k, y, :x0] = 0; planes[n, k, y, x1:] = 0
    return planes, wins


def yolact_device_window(box, PH, PW, h, w, slack=2):
    """yolact_upsample_masks_kernel's window arithmetic in fp32 (slack: its +- 2 output pixels); slack = None: the whole image"""
    if slack is None:
        return (0, 0, w, h)
    x1, x2, y1, y2 = yolact_crop(box, PH, PW)
    out = []
    for lo, hi, in_sz, out_sz in ((x1, x2, PW, w), (y1, y2, PH, h)):
        fs = F32(out_sz) / F32(in_sz)
        a = int(np.floor(F32(F32(np.ceil(lo) - F32(1.0) + F32(0.5)) * fs) - F32(0.5))) - slack
        b = int(np.ceil(F32(F32(np.ceil(hi) + F32(0.5)) * fs) - F32(0.5))) + slack
        out.append((max(a, 0), min(b, out_sz)))
    return (out[0][0], out[1][0], out[0][1], out[1][1])


def model_yolact(case, dense, planes, wins, mutate=None):
    """what yolact_upsample_masks_kernel leaves with clear = 0: per live slot the conservative window and byte stores inside it alone.
    mutate: 'tight' (the computed bound with one pixel cut off instead of two added), 'whole_plane' (every window is the image), 'window_short_row' (reports
    y1 - 1), 'skip_last_row' (does not store the window's last row)"""
    planes, wins = planes.copy(), wins.copy()
    hw = image_sizes(case)
    for n in range(planes.shape[0]):
        hn, wn = int(hw[n, 0]), int(hw[n, 1])
        for k in range(int(case["counts"][n])):
            slack = {"tight": -1, "whole_plane": None}.get(mutate, 2)
            x0, y0, x1, y1 = yolact_device_window(case["boxes"][n, k], case["PH"], case["PW"], hn, wn, slack)
            wins[n, k] = (x0, y0, x1, y1 - 1 if mutate == "window_short_row" else y1)
            if x1 > x0 and y1 > y0:
                ys = y1 - 1 if mutate == "skip_last_row" else y1
                planes[n, k, y0:ys, x0:x1] = dense[n, k, y0:ys, x0:x1]
    return planes, wins


# ------------------------------------------------------------------------------------------------------------------ mask-IoU net ends
def fmaf(a, b, c):
    """fp32 fused multiply-add of arrays, exactly: the fp32 product is exact in fp64; the fp64 sum is rounded to odd (its error term from the two-sum),
    after which the rounding to fp32 is the single rounding of the exact a * b + c (53 >= 2 * 24 + 2 bits)"""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def maskiou_conv1_ref(lo, w, b):
    """-> (fp32 restatement of the kernel's chain [NK, Ho, Wo, 8], fp64 value before the ReLU, sum |x w| + |b|): nine chained fmaf over the taps in
    row-major order from 0, fmaf(acc, 1, bias), + 0, ReLU"""
    lo = np.asarray(lo, F32); w = np.asarray(w, F32).reshape(8, 9); b = np.asarray(b, F32).reshape(8)
    NK, PH, PW = lo.shape
    Ho, Wo = (PH - 3) // 2 + 1, (PW - 3) // 2 + 1
    taps = np.stack([lo[:, r:r + 2 * Ho - 1:2, c:c + 2 * Wo - 1:2] for r in range(3) for c in range(3)], -1)     # [NK, Ho, Wo, 9]
    acc = np.zeros((NK, Ho, Wo, 8), F32)
    for k in range(9):
        acc = fmaf(taps[..., k:k + 1], w[None, None, None, :, k], acc)
    v = fmaf(acc, F32(1.0), b) + F32(0.0)
    exact = taps.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    mag = np.abs(taps.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
    return np.where(v > 0, v, F32(0.0)).astype(F32), exact, mag
