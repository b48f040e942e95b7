"""The painter's contract in numpy (csrc/render.hip computes the same thing pixel-parallel), written as the per-entry loop the host overlays
are, and the case builders the CPU and GPU tests share.

    entries int32 [D, 8] = {slot, x1, y1, x2, y2, colour, flags, 0}      dots int32 [Q, 4] = {x, y, colour, half}
    masks uint8 [slots, ph, pw], the image in each plane's top-left H x W, a byte != 0 is set
"""
import numpy as np

VALUES = np.array([0, 1, 2, 255], np.uint8)   # mask bytes: clear, the usual 1, and two other ways of being set


def unpack_color(c):
    return np.array([c & 255, (c >> 8) & 255, (c >> 16) & 255], np.uint8)


def paint_ref(image, masks, entries, dots):
    out = np.array(image, np.uint8)
    H, W = out.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    entries, dots = ([] if entries is None else entries), ([] if dots is None else dots)
    for slot, x1, y1, x2, y2, colour, flags, _ in np.asarray(entries, np.int64).reshape(-1, 8).tolist():
        c = unpack_color(colour)
        if slot >= 0:
            m = masks[slot, :H, :W] != 0
            out[m] = ((out[m].astype(np.uint16) + c.astype(np.uint16)) >> 1).astype(np.uint8)
        if flags & 1:
            on = ((y1 <= ys) & (ys <= y2) & ((xs == x1) | (xs == x2))) | ((x1 <= xs) & (xs <= x2) & ((ys == y1) | (ys == y2)))
            out[on] = c
    for x, y, colour, half in np.asarray(dots, np.int64).reshape(-1, 4).tolist():
        if abs(y) > H + 16:   # cannot reach the image (a speed-up of this loop only)
            continue
        on = (np.abs(xs - x) <= half) & (np.abs(ys - y) <= half)
        out[on] = unpack_color(colour)
    return out


def plane_shape(H, W, pw_extra):
    """ph > H, pw = W + pw_extra; where pw is odd ph is made odd too, so ph * pw is odd and every second plane starts on an odd byte"""
    pw = W + pw_extra
    ph = H + 1
    if pw % 2 == 1 and ph % 2 == 0:
        ph += 1
    return ph, pw


def random_image(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def overlap_case(seed, H, W, pw_extra, D, slots=5):
    """D entries that ALL touch one pixel (cx, cy): masked entries through their planes (set there), box-only entries through an outline that passes it.
    Slots repeat, come out of order and mix with -1; mask bytes from VALUES; boxes reach up to two pixels outside the image.
    -> image, masks, entries, (cx, cy)"""
    rng = np.random.default_rng(seed)
    ph, pw = plane_shape(H, W, pw_extra)
    masks = VALUES[rng.integers(0, 4, (slots, ph, pw))]
    cx, cy = int(rng.integers(0, W)), int(rng.integers(0, H))
    masks[:, cy, cx] = VALUES[rng.integers(1, 4, slots)]
    e = np.zeros((D, 8), np.int32)
    e[:, 0] = rng.integers(-1, slots, D)
    e[:, 1] = rng.integers(-2, W + 2, D); e[:, 3] = rng.integers(-2, W + 2, D)
    e[:, 2] = rng.integers(-2, H + 2, D); e[:, 4] = rng.integers(-2, H + 2, D)
    e[:, 5] = rng.integers(0, 1 << 24, D)
    e[:, 6] = rng.integers(0, 2, D)
    for k in np.nonzero(e[:, 0] < 0)[0]:   # a box-only entry reaches (cx, cy) through its left edge
        e[k, 1], e[k, 2], e[k, 4], e[k, 6] = cx, min(e[k, 2], cy), max(e[k, 4], cy), 1
    return random_image(rng, H, W), masks, e, (cx, cy)


def outline_entries(H, W):
    """(name, entry) of every outline form of the contract, each in its own colour"""
    forms = [("image edges", (0, 0, W - 1, H - 1), 1),
             ("one pixel wide", (W // 2, 0, W // 2, H - 1), 1),
             ("one pixel high", (0, H // 2, W - 1, H // 2), 1),
             ("one pixel", (W - 1, H - 1, W - 1, H - 1), 1),
             ("y2 < y1", (0, H - 1, W - 1, 0), 1),          # rows y1 and y2 over x1..x2 still paint, no column does
             ("x2 < x1", (W - 1, 0, 0, H - 1), 1),
             ("outside left/top", (-5, -4, -1, -1), 1),
             ("outside right/bottom", (W, H, W + 3, H + 2), 1),
             ("spans the image from outside", (-1, -1, W, H), 1),   # every edge one pixel outside: nothing painted
             ("left edge outside", (-1, 0, W - 1, H - 1), 1),
             ("flag off", (0, 0, W - 1, H - 1), 0)]
    return [(n, np.array([-1, *b, 0x102030 + 0x0F0709 * i, f, 0], np.int32)) for i, (n, b, f) in enumerate(forms)]


def dot_cases(H, W):
    """(name, dots [q, 4]): corners, one pixel outside each side, half 0 and 8"""
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    outside = [(-1, H // 2), (W, H // 2), (W // 2, -1), (W // 2, H)]
    out = []
    for half in (0, 2, 8):
        out.append(("corners half %d" % half, np.array([(x, y, 0x0000FF + 0x010100 * i, half) for i, (x, y) in enumerate(corners)], np.int32)))
        out.append(("outside half %d" % half, np.array([(x, y, 0x00FF00 + 0x010001 * i, half) for i, (x, y) in enumerate(outside)], np.int32)))
    out.append(("just out of reach", np.array([(-9, 0, 0xFFFFFF, 8), (W + 8, 0, 0xFFFFFF, 8), (0, -9, 0xFFFFFF, 8), (0, H + 8, 0xFFFFFF, 8)], np.int32)))
    return out


def many_dots(seed, H, W, Q):
    """Q dots, most of them off the image (the row test skips them), the rest overlapping each other in order"""
    rng = np.random.default_rng(seed)
    d = np.zeros((Q, 4), np.int32)
    d[:, 0] = rng.integers(-12, W + 12, Q)
    d[:, 1] = rng.integers(-40, H + 40, Q)
    d[:, 2] = rng.integers(0, 1 << 24, Q)
    d[:, 3] = rng.integers(0, 9, Q)
    return d


def planes_of(masks_hw, ph, pw):
    """[n, H, W] masks -> [n, ph, pw] planes, the padding filled with 255 (a painter that read it would show)"""
    m = np.asarray(masks_hw, np.uint8)
    p = np.full((m.shape[0], ph, pw), 255, np.uint8)
    p[:, :m.shape[1], :m.shape[2]] = m
    return p


def crafted_predictions(seed, H, W, n, keypoints=False, with_masks=True):
    """A BoxList as COCODemo.overlay takes it: overlapping blob masks, boxes that reach past the image (the overlay clamps them), scores, labels, `slot`."""
    from isegmi.maskrcnn import BoxList
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(-3, W * 0.6, n); y1 = rng.uniform(-3, H * 0.6, n)
    box = np.stack([x1, y1, x1 + rng.uniform(1, W * 0.7, n), y1 + rng.uniform(1, H * 0.7, n)], 1).astype(np.float32)
    bl = BoxList(box, (W, H))
    bl.add_field("scores", rng.uniform(0.3, 1.0, n).astype(np.float32))
    bl.add_field("labels", rng.integers(1, 81, n).astype(np.int64))
    bl.add_field("slot", rng.permutation(n).astype(np.int64))
    if with_masks:
        ys, xs = np.mgrid[0:H, 0:W]
        m = np.zeros((n, 1, H, W), np.uint8)
        for k in range(n):
            bx1, by1, bx2, by2 = box[k]
            m[k, 0] = ((xs - (bx1 + bx2) / 2) ** 2 / max((bx2 - bx1) / 2, 1) ** 2 + (ys - (by1 + by2) / 2) ** 2 / max((by2 - by1) / 2, 1) ** 2) <= 1.0
        bl.add_field("mask", m)
    if keypoints:
        kp = np.zeros((n, 17, 3), np.float32)
        kp[..., 0] = rng.uniform(-3, W + 3, (n, 17)); kp[..., 1] = rng.uniform(-3, H + 3, (n, 17)); kp[..., 2] = 1
        kp[0, 0, :2] = (0.4, 0.6); kp[0, 1, :2] = (W - 1, H - 1)   # dots clipped at two corners
        bl.add_field("keypoints", kp)
        bl.add_field("keypoint_logits", rng.uniform(0.0, 4.0, (n, 17)).astype(np.float32))
    return bl


def slot_planes(predictions, ph, pw):
    """the planes det.masks would hold for crafted_predictions: row `slot` of the buffer is that prediction's mask"""
    m = predictions.get_field("mask")[:, 0]
    p = np.full((len(predictions), ph, pw), 255, np.uint8)
    for k, s in enumerate(predictions.get_field("slot")):
        p[s, :m.shape[1], :m.shape[2]] = m[k]
    return p
