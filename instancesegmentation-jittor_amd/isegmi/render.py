"""Draw lists of the device painter (csrc/render.hip, isegmi_op_paint / isegmi_engine_paint).

The host overlays stay the contract -- COCODemo.overlay / overlay_keypoints for the R-CNN family, cli._overlay for Yolact; the builders here turn the same
detections into the same integers those loops use, so the painter's image equals theirs bit for bit:
    entries int32 [D, 8] = {slot, x1, y1, x2, y2, colour, flags, 0}     slot: the detection's row of det.masks (-1: box only); flags bit 0: outline
    dots    int32 [Q, 4] = {x, y, colour, half}
colour = c0 | c1 << 8 | c2 << 16, the three channel bytes in the image's own order.
"""
import numpy as np

MAX_ENTRIES, MAX_DOTS, MAX_HALF = 1024, 32768, 8
OUTLINE = 1
KEYPOINT_HALF = 2   # overlay_keypoints' 5 x 5 dot


def pack_colors(colors_u8):
    """[n, 3] uint8 channel bytes -> [n] int32 c0 | c1 << 8 | c2 << 16"""
    c = np.asarray(colors_u8, np.uint8).reshape(-1, 3).astype(np.int32)
    return c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)


def make_entries(slots, boxes_int, colors_u8, outline=True):
    """One entry per detection, in drawing order.  boxes_int [n, 4]: the outline's x1, y1, x2, y2 as the host loop indexes them."""
    n = len(slots)
    e = np.zeros((n, 8), np.int32)
    if n:
        e[:, 0] = np.asarray(slots, np.int64)
        e[:, 1:5] = np.asarray(boxes_int, np.int64).reshape(n, 4)
        e[:, 5] = pack_colors(colors_u8)
        e[:, 6] = OUTLINE if outline else 0
    if n > MAX_ENTRIES:
        raise ValueError("a draw list holds at most %d entries (%d given)" % (MAX_ENTRIES, n))
    return e


def demo_entries(predictions, H, W, with_masks=True):
    """COCODemo.overlay's loop as a draw list: int() of the box, both corners clamped into the image, compute_colors_for_labels colours; slot = the
    prediction's `slot` field (its row before select_top_predictions), -1 for a model without masks."""
    from .predictor import COCODemo
    n = len(predictions)
    colors = COCODemo.compute_colors_for_labels(predictions.get_field("labels")) if n else np.zeros((0, 3), np.uint8)
    boxes = np.zeros((n, 4), np.int64)
    for k in range(n):
        x1, y1, x2, y2 = (int(v) for v in predictions.bbox[k])
        boxes[k] = (max(0, min(W - 1, x1)), max(0, min(H - 1, y1)), max(0, min(W - 1, x2)), max(0, min(H - 1, y2)))
    slots = np.asarray(predictions.get_field("slot"), np.int64) if with_masks else np.full(n, -1, np.int64)
    return make_entries(slots, boxes, colors)


def keypoint_dots(predictions, kp_thresh):
    """COCODemo.overlay_keypoints' loop as a dot list: every keypoint whose logit exceeds kp_thresh, detection by detection, coloured by joint."""
    from .predictor import COCODemo
    kps, logits = predictions.get_field("keypoints"), predictions.get_field("keypoint_logits")
    colors = pack_colors(COCODemo.compute_colors_for_labels(np.arange(1, kps.shape[1] + 1)))
    rows = []
    for k in range(len(predictions)):
        for j in np.nonzero(logits[k] > kp_thresh)[0]:
            rows.append((int(kps[k, j, 0]), int(kps[k, j, 1]), int(colors[j]), KEYPOINT_HALF))
    if len(rows) > MAX_DOTS:
        raise ValueError("a dot list holds at most %d dots (%d given)" % (MAX_DOTS, len(rows)))
    return np.asarray(rows, np.int32).reshape(-1, 4)


def yolact_entries(slots, boxes, classes, H, W):
    """cli._overlay's loop as a draw list: int() of the box, x2 / y2 clamped to W-1 / H-1, colours of class + 1."""
    from .predictor import COCODemo
    n = len(classes)
    colors = COCODemo.compute_colors_for_labels(np.asarray(classes) + 1) if n else np.zeros((0, 3), np.uint8)
    b = np.zeros((n, 4), np.int64)
    for k in range(n):
        x1, y1, x2, y2 = (int(v) for v in boxes[k])
        b[k] = (x1, y1, min(x2, W - 1), min(y2, H - 1))
    return make_entries(slots, b, colors)
