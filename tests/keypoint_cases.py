"""Inputs of the Keypoint R-CNN tests (TEST INFRASTRUCTURE ONLY; tests/test_keypointrcnn_cpu.py, tests/test_keypoint_ops_gpu.py,
tests/test_keypointrcnn_gpu.py): the smooth-peak maps of the second-opinion test, the crafted detections of the decode kernel's edges, the batches
built from them with their restated results (computed once per process, never modified), and the keypoint block's size from its definition."""
import functools

import numpy as np

import keypoint_ref as kr

S, K = 56, 17
F = np.float32

TORCH_SIZES = ((1, 1), (1, 57), (2, 3), (55, 56), (56, 56), (57, 113), (200, 90), (331, 7), (640, 480))   # (hc, wc) of the second-opinion test


def smooth_peak_maps(seed=0, k=K, s=S):
    """[s, s, k]: per channel a Gaussian of height 8, sigma 3 px at a random centre, plus 0.05 N(0, 1) noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(s, dtype=np.float64), np.arange(s, dtype=np.float64), indexing="ij")
    out = np.empty((s, s, k), F)
    for c in range(k):
        cy, cx = rng.uniform(0, s - 1, 2)
        out[:, :, c] = 8.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 3.0 ** 2)) + 0.05 * rng.standard_normal((s, s))
    return out


BLOB = np.array([[1.0, 2.0, 1.5], [2.5, 8.0, 3.0], [1.25, 3.5, 2.25]], F)   # asymmetric: its enlarged maximum is one position, not a symmetric pair


def _blob_maps(centres):
    """[S, S, K] zero maps with BLOB pasted at every (y, x) of `centres`, moved by (k % 5, k % 7) in channel k: a wrong channel stride shows."""
    m = np.zeros((S, S, K), F)
    for k in range(K):
        for y, x in centres:
            yy, xx = y + k % 5, x + k % 7
            m[yy - 1:yy + 2, xx - 1:xx + 2, k] = BLOB
    return m


def _point_maps(points, value=8.0):
    m = smooth_peak_maps(3) * F(0.125)   # a low background, so that the planted value is the maximum
    for k in range(K):
        y, x = points(k)
        m[y, x, k] = value
    return m


# name -> (box, maps [S, S, K]); boxes have non-zero, non-integer origins (the canvas-sized one starts at a quarter pixel)
def detections():
    d = {}
    d["tiny"] = ((10.3, 20.7, 10.8, 21.1), smooth_peak_maps(1))                      # w, h < 1: a 1 x 1 output
    d["1x57"] = ((3.25, 4.5, 3.75, 61.5), smooth_peak_maps(2))                       # wc 1, hc 57
    d["identity"] = ((7.5, 9.25, 63.5, 65.25), smooth_peak_maps(4))                  # exactly 56 x 56: t = 0, weights (0, 1, 0, 0)
    d["55.5x56.25"] = ((1.5, 2.25, 57.0, 58.5), smooth_peak_maps(5))                 # wc 56 with cw < 1, hc 57
    d["tie"] = ((12.5, 6.75, 124.5, 118.75), _blob_maps(((30, 10), (20, 30))))       # 112 x 112, two identical peaks (10, -20) source pixels apart
    d["zero"] = ((5.5, 6.5, 45.25, 30.75), np.zeros((S, S, K), F))                   # all-zero maps: position 0
    d["last"] = ((2.5, 3.5, 114.5, 87.5), _point_maps(lambda k: (S - 1, S - 1)))      # maximum at the bottom-right position
    d["border"] = ((8.25, 4.75, 176.25, 172.75), _point_maps(lambda k: (0, 5 + 2 * k)))   # x3: maximum in the top band, where the taps are clamped
    d["canvas"] = ((0.25, 0.5, 1344.0, 800.0), smooth_peak_maps(6))                  # 800 x 1344 output: 1.07 M positions per map
    return d


def block_bytes(n, cap, nk=K):
    """Size of the keypoint record block from its definition: 16 status bytes, n*cap boxes of 16, n counts, n*cap scores, n*cap labels of 4, n*cap*nk
    keypoints of 12 and n*cap*nk logits of 4, every section padded to a multiple of 8."""
    r8 = lambda v: -(-v // 8) * 8
    return 16 + r8(n * cap * 16) + r8(n * 4) + r8(n * cap * 4) + r8(n * cap * 4) + r8(n * cap * nk * 12) + r8(n * cap * nk * 4)


def _batch(N, cap, slots):
    """slots: {(n, c): (box, maps)} -> heat [N * cap, S, S, K] and boxes [N, cap, 4] (NaN wherever no detection sits: an empty slot that is read shows), count [N]"""
    heat = np.full((N * cap, S, S, K), np.nan, F)
    boxes = np.full((N, cap, 4), np.nan, F)
    count = np.zeros(N, np.int32)
    for (n, c), (box, maps) in slots.items():
        heat[n * cap + c] = maps
        boxes[n, c] = box
        count[n] = max(count[n], c + 1)
    return heat, boxes, count


@functools.lru_cache(maxsize=None)
def decode_batch(cap):
    """-> (heat, boxes, count, want_kpt, want_kscore), read-only.  cap 7: N = 3 with a full image (the seven small edge cases), an image with count 0 and
    one with two detections (border, canvas); cap 1: N = 2, one detection and an empty image; cap 100: N = 1, 37 smooth-peak detections of moderate size."""
    d = detections()
    if cap == 7:
        names = ("tiny", "1x57", "identity", "55.5x56.25", "tie", "zero", "last")
        slots = {(0, i): d[k] for i, k in enumerate(names)}
        slots[(2, 0)] = d["border"]; slots[(2, 1)] = d["canvas"]
        N = 3
    elif cap == 1:
        slots, N = {(0, 0): d["55.5x56.25"]}, 2
    elif cap == 100:
        rng = np.random.default_rng(100)
        slots, N = {}, 1
        for c in range(37):
            x1, y1 = rng.uniform(0.5, 300.0, 2)
            w, h = rng.uniform(0.5, 140.0, 2)
            slots[(0, c)] = ((x1, y1, x1 + w, y1 + h), smooth_peak_maps(1000 + c))
    else:
        raise KeyError(cap)
    heat, boxes, count = _batch(N, cap, slots)
    kpt, ks = kr.decode(heat, boxes, count)
    for a in (heat, boxes, count, kpt, ks):
        a.setflags(write=False)
    return heat, boxes, count, kpt, ks
