"""COCO-format results: bbox xywh, category-id remap and RLE mask encoding.

The reference reaches this through `python tools/test_net.py` -> inference() -> COCO json (README.md:344-347)
and Yolact eval.py's Detections.add_bbox/add_mask/dump (README.md:243-249); annotation layout README.md:55-66.
pycocotools is not in the image, so the run-length encoder and its LEB128-style string compression
(pycocotools maskApi.c rleEncode / rleToString / rleFrString) are restated here in numpy/Python.
"""
import json

import numpy as np

# contiguous label 1..80 -> COCO category id (the 2017 "thing" classes)
COCO_CATEGORY_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34,
                     35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65,
                     67, 70, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90]
COCO_CLASSES = ("person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light", "fire hydrant",
                "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe",
                "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard", "sports ball", "kite", "baseball bat",
                "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl",
                "banana", "apple", "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch",
                "potted plant", "bed", "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave",
                "oven", "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush")


def rle_counts(mask):
    """Column-major run lengths of a binary HxW mask, starting with the count of zeros (rleEncode)."""
    m = np.asarray(mask).astype(bool)
    flat = m.ravel(order="F")
    if flat.size == 0:
        return [0]
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    bounds = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(bounds).tolist()
    if flat[0]:
        counts = [0] + counts
    return counts


def rle_to_string(counts):
    """pycocotools rleToString: delta vs the count two runs back, 5 data bits + continuation bit per char."""
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_from_string(s):
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_encode(mask):
    h, w = np.asarray(mask).shape
    return {"size": [int(h), int(w)], "counts": rle_to_string(rle_counts(mask))}


def rle_decode(rle):
    h, w = rle["size"]
    counts = rle_from_string(rle["counts"]) if isinstance(rle["counts"], str) else list(rle["counts"])
    flat = np.zeros(h * w, np.uint8)
    pos, val = 0, 0
    for c in counts:
        if val:
            flat[pos:pos + c] = 1
        pos += c
        val ^= 1
    return flat.reshape((h, w), order="F")


def rle_from_polygon(xy, h, w):
    """Run counts (column-major, zeros first) of one polygon [x0, y0, x1, y1, ...] in an h x w image.
    [UPSTREAM-RECALL -- unverified] pycocotools maskApi.c rleFrPoly: vertices scaled by 5 and rounded with +0.5 truncation; every edge walked one
    step along its longer axis with the other coordinate rounded; the points where x changes mapped back with (x + 0.5) / 5 - 0.5, kept where
    that is an integer column inside the image, y clamped to [0, h] and rounded up; the flat positions x * h + y sorted, h * w appended,
    differenced, and zero-length runs folded into their neighbours."""
    xy = np.asarray(xy, np.float64).ravel()
    k = xy.size // 2
    h, w = int(h), int(w)
    if k == 0:
        return [h * w]
    scale = 5.0
    x = np.trunc(scale * xy[0:2 * k:2] + 0.5).astype(np.int64)
    y = np.trunc(scale * xy[1:2 * k:2] + 0.5).astype(np.int64)
    x = np.append(x, x[0]); y = np.append(y, y[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(x[j]), int(x[j + 1]), int(y[j]), int(y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0     # a degenerate edge (dx = dy = 0) is 0 / 0 upstream; it contributes its single point
            t = np.arange(dx, -1, -1) if flip else np.arange(dx + 1)
            us.append(t + xs)
            vs.append(np.trunc(ys + s * t + 0.5).astype(np.int64))
        else:
            s = (xe - xs) / dy
            t = np.arange(dy, -1, -1) if flip else np.arange(dy + 1)
            vs.append(t + ys)
            us.append(np.trunc(xs + s * t + 0.5).astype(np.int64))
    u = np.concatenate(us); v = np.concatenate(vs)
    # the points where x changes: the y-boundary crossings, mapped back to pixel columns
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    ch = u1 != u0
    u0, u1, v0, v1 = u0[ch], u1[ch], v0[ch], v1[ch]
    xd = np.where(u1 < u0, u1, u1 - 1).astype(np.float64)
    xd = (xd + 0.5) / scale - 0.5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.where(v1 < v0, v1, v0).astype(np.float64)
    yd = (yd + 0.5) / scale - 0.5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    a = (xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64))
    a = np.sort(np.append(a, h * w))
    d = np.diff(np.concatenate([[0], a])).tolist()
    # fold zero-length runs: a zero count joins its two neighbours into one run
    b = [d[0]]
    j = 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j]); j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]; j += 1
    return b


def _rle_intervals(counts):
    """[start, end) of the 1-runs of a count list, empty ones dropped."""
    c = np.asarray(counts, np.int64).ravel()
    e = np.cumsum(c)
    s = e - c
    s, e = s[1::2], e[1::2]
    nz = e > s
    return s[nz], e[nz]


def rle_merge(counts_list, hw_pixels):
    """Union of several RLEs of one image size (hw_pixels = h * w) as canonical run counts.
    [UPSTREAM-RECALL -- unverified] the result of pycocotools rleMerge(intersect=0): the parts of one annotation joined into one mask."""
    parts = [_rle_intervals(c) for c in counts_list]
    s = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.int64)
    e = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
    if s.size == 0:
        return [int(hw_pixels)]
    o = np.argsort(s, kind="stable")
    s, e = s[o], e[o]
    reach = np.maximum.accumulate(e)
    first = np.ones(s.size, bool)
    first[1:] = s[1:] > reach[:-1]          # touching or overlapping intervals are one run
    starts = s[first]
    ends = np.append(reach[:-1][first[1:]], reach[-1])
    b = np.empty(2 * starts.size + 1, np.int64)
    b[0:-1:2] = starts; b[1::2] = ends; b[-1] = int(hw_pixels)
    out = np.diff(np.concatenate([[0], b])).tolist()
    if out[-1] == 0:
        out.pop()
    return out


def rle_area(counts):
    """Set pixels of a count list (rleArea)."""
    return int(np.asarray(counts, np.int64).ravel()[1::2].sum())


def rle_to_bbox(counts, h):
    """Tight box [x, y, w, h] of a count list (rleToBbox), [0, 0, 0, 0] for an empty mask.  Empty 1-runs are skipped."""
    s, e = _rle_intervals(counts)
    if s.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    h = int(h)
    last = e - 1
    xs, xe = s // h, last // h
    wrap = xs < xe
    if wrap.any():
        y0, y1 = 0, h - 1
    else:
        y0, y1 = int((s - xs * h).min()), int((last - xe * h).max())
    x0, x1 = int(xs.min()), int(xe.max())
    return [float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)]


def label_categories(num_classes=81, category_ids=None):
    """The json category id of every contiguous label 1 .. num_classes - 1, as a list indexed by label (entry 0, the background, is None).
    category_ids given: its entry label - 1 (a data set's own contiguous -> json id map; it must name num_classes - 1 ids).  Otherwise 81 classes map
    to the COCO ids (COCO_CATEGORY_IDS), and for any other class count the label IS the category id."""
    n = int(num_classes)
    if category_ids is not None:
        ids = [int(c) for c in category_ids]
        if len(ids) != n - 1:
            raise ValueError("category_ids names %d ids, the model has %d classes besides the background" % (len(ids), n - 1))
        return [None] + ids
    return [None] + (list(COCO_CATEGORY_IDS) if n == 81 else list(range(1, n)))


def maskrcnn_results(image_id, boxes_xyxy, scores, labels, masks=None, categories=None, keypoints=None):
    """maskrcnn-benchmark prepare_for_coco_detection/segmentation: bbox xywh with the legacy +1 widths,
    category_id via the contiguous->json id map (categories: a label_categories() list; default the 80 COCO classes), segmentation = RLE of the
    pasted HxW mask (masks None: bbox-only results, no `segmentation` key).  keypoints [n, NK, 3] (Keypoint R-CNN): every entry also
    carries `keypoints`, the NK * 3 numbers x, y, v of prepare_for_coco_keypoint -- ONE entry per detection where upstream writes a bbox and a keypoint file."""
    out = []
    b = np.asarray(boxes_xyxy, np.float32).reshape(-1, 4)
    cats = categories if categories is not None else label_categories()
    for k in range(b.shape[0]):
        x1, y1, x2, y2 = (float(v) for v in b[k])
        d = {"image_id": int(image_id), "category_id": cats[int(labels[k])],
             "bbox": [x1, y1, x2 - x1 + 1.0, y2 - y1 + 1.0], "score": float(scores[k])}
        if masks is not None:
            d["segmentation"] = rle_encode(masks[k])
        if keypoints is not None:
            d["keypoints"] = np.asarray(keypoints[k], np.float64).reshape(-1).tolist()
        out.append(d)
    return out


def yolo_results(image_id, boxes_xyxy, scores, labels, categories=None):
    """YOLOv3 bbox-only COCO entries: bbox = (x1, y1, x2 - x1, y2 - y1), plain widths (no +1); category_id through the contiguous -> json id map
    (categories: a label_categories() list; default the 80 COCO classes)."""
    cats = categories if categories is not None else label_categories()
    b = np.asarray(boxes_xyxy, np.float32).reshape(-1, 4)
    out = []
    for k in range(b.shape[0]):
        x1, y1, x2, y2 = (float(v) for v in b[k])
        out.append({"image_id": int(image_id), "category_id": cats[int(labels[k])], "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(scores[k])})
    return out


def yolact_results(image_id, classes, scores, boxes_xyxy_int, masks=None, mask_scores=None):
    """Yolact eval.py Detections.add_bbox/add_mask: bbox [x1,y1,w,h] rounded to 0.1, class 0..79 -> COCO id.
    mask_scores (YOLACT++ re-scoring): upstream writes the mask entry with the re-scored value; kept here as "mask_score"."""
    out = []
    b = np.asarray(boxes_xyxy_int).reshape(-1, 4)
    for k in range(b.shape[0]):
        x1, y1, x2, y2 = (float(v) for v in b[k])
        bbox = [round(v * 10) / 10 for v in (x1, y1, x2 - x1, y2 - y1)]
        d = {"image_id": int(image_id), "category_id": COCO_CATEGORY_IDS[int(classes[k])], "bbox": bbox, "score": float(scores[k])}
        if masks is not None:
            d["segmentation"] = rle_encode(masks[k])
        if mask_scores is not None:
            d["mask_score"] = float(mask_scores[k])
        out.append(d)
    return out


def results_from_records(rec, image_ids, image_hw, kind, K=100, score_threshold=None, top_k=None, categories=None):
    """One rank's unpacked record block (isegmi.dist.unpack_coco_records: the device-side output of a step) -> COCO result dicts, the
    same records maskrcnn_results / yolact_results build from host arrays: bbox conversion and category map here, `segmentation.counts`
    straight from the device-made strings.  image_ids / image_hw: per image slot of the batch (None id = an empty padding slot).
    score_threshold / top_k (Yolact eval.py --score_threshold / --top_k): keep score > threshold, then the first top_k (score order).
    kind: 1 Yolact, 2 Mask R-CNN, 3 Pose2Seg (category 1, bbox = the mask's tight box; the score is the record's, like every kind's: 1.0 as
    isegmi_pose2seg_forward writes it, the detection's box score from a KeypointPose2Seg step).  A box-only block (Faster R-CNN: no str_off in
    `rec`) gives bbox-only results without a `segmentation` key; a keypoint block (Keypoint R-CNN: `kpt` in `rec`) adds `keypoints`, NK * 3 numbers x, y, v.
    categories (kind 2): a label_categories() list, default the 80 COCO classes."""
    out = []
    count, box, score, label = rec["count"], rec["box"], rec["score"], rec["label"]
    so, chars = rec.get("str_off"), rec.get("chars")
    lab_cat = categories if categories is not None else label_categories()
    ms, kp = rec.get("mscore"), rec.get("kpt")
    for n, iid in enumerate(image_ids):
        c = int(count[n])
        if iid is None or c == 0:
            continue
        h, w = int(image_hw[n][0]), int(image_hw[n][1])
        b = np.asarray(box[n, :c], np.float64)
        if kind == 3:   # Pose2Seg test.py: every person is category 1; the tight mask box (right / bottom exclusive) as xywh
            bb = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).tolist()
            cats = [1] * c
        elif kind == 2:   # prepare_for_coco_detection: xyxy -> xywh with the legacy +1
            bb = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + 1.0, b[:, 3] - b[:, 1] + 1.0], 1).tolist()
            cats = [lab_cat[int(l)] for l in label[n, :c]]
        else:           # Detections.add_bbox: [x1, y1, w, h] rounded to 0.1
            bb = (np.round(np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1) * 10) / 10).tolist()
            cats = [COCO_CATEGORY_IDS[int(l)] for l in label[n, :c]]
        sc = np.asarray(score[n, :c], np.float64).tolist()
        offs = so[n * K:n * K + c + 1].tolist() if so is not None else None
        keep = range(c)
        if score_threshold is not None:
            keep = [k for k in keep if score[n, k] > np.float32(score_threshold)]
        if top_k is not None:
            keep = list(keep)[:top_k]
        for k in keep:
            d = {"image_id": int(iid), "category_id": cats[k], "bbox": bb[k], "score": sc[k]}
            if offs is not None:
                d["segmentation"] = {"size": [h, w], "counts": chars[offs[k]:offs[k + 1]].decode("ascii")}
            if ms is not None:
                d["mask_score"] = float(ms[n, k])
            if kp is not None:
                d["keypoints"] = np.asarray(kp[n, k], np.float64).reshape(-1).tolist()
            out.append(d)
    return out


def dump(results, path):
    with open(path, "w") as f:
        json.dump(results, f)
