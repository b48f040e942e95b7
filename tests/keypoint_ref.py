"""numpy restatement of the Keypoint R-CNN tail (TEST INFRASTRUCTURE ONLY): the fused bicubic resize + arg-max of isegmi_op_keypoint_decode,
the pixel shuffle + bilinear x2 of isegmi_op_keypoint_heatmap, the keypoint head stage by stage and the keypoint record block.

THE ARITHMETIC.  The library is built with -ffp-contract=off and the decode kernel is written with plain `*` and `+`, so numpy's elementwise fp32
operations, applied in the same order, give the same bits: every line below that touches a float32 array is ONE rounded fp32 operation per element.
    f = (d + 0.5) * (n_in / n_out) - 0.5,  s = floor(f),  t = f - s,  u = 1 - t,  x = t + 1,  A = -0.75
    w0 = ((A x - 5A) x + 8A) x - 4A;  w1 = ((A+2) t - (A+3)) t t + 1;  w2 = the same in u;  w3 = 1 - w0 - w1 - w2
    taps clamp(s-1 .. s+2, 0, n_in - 1); horizontal pass first, both passes summed left to right.
The bilinear half is the oracle's (ora.resize_bilinear), whose rounding sequence oracle/ora_ops.c states.
"""
import numpy as np

from oracle import ora

F = np.float32
A = F(-0.75)
A5, A8, A4, A2, A3 = F(-3.75), F(-6.0), F(-3.0), F(1.25), F(2.25)
MAX_SIDE = 16384


def cubic_taps(n_out, n_in):
    """-> (idx [n_out, 4] clamped tap indices, w [n_out, 4] fp32 weights)"""
    d = np.arange(n_out, dtype=F)
    scale = F(n_in) / F(n_out)
    f = (d + F(0.5)) * scale - F(0.5)
    sf = np.floor(f)
    t = f - sf
    u = F(1.0) - t
    x = t + F(1.0)
    w0 = ((A * x - A5) * x + A8) * x - A4
    w1 = ((A2 * t - A3) * t) * t + F(1.0)
    w2 = ((A2 * u - A3) * u) * u + F(1.0)
    w3 = ((F(1.0) - w0) - w1) - w2
    s = sf.astype(np.int64)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    w = np.stack([w0, w1, w2, w3], 1)
    assert w.dtype == F
    return idx, w, s


def resize_bicubic(m, hc, wc):
    """m [S, S] fp32 -> [hc, wc] fp32: cv2.INTER_CUBIC's two passes in fp32."""
    m = np.ascontiguousarray(m, F)
    S = m.shape[0]
    xi, wx, _ = cubic_taps(wc, S)
    yi, wy, _ = cubic_taps(hc, S)
    rows = ((wx[:, 0] * m[:, xi[:, 0]] + wx[:, 1] * m[:, xi[:, 1]]) + wx[:, 2] * m[:, xi[:, 2]]) + wx[:, 3] * m[:, xi[:, 3]]   # [S, wc]
    out = ((wy[:, 0, None] * rows[yi[:, 0]] + wy[:, 1, None] * rows[yi[:, 1]]) + wy[:, 2, None] * rows[yi[:, 2]]) + wy[:, 3, None] * rows[yi[:, 3]]
    assert out.dtype == F and out.shape == (hc, wc)
    return out


def box_sizes(box):
    """-> (w, h fp32, wc, hc int) of heatmaps_to_keypoints: widths without +1, at least 1, ceil; resized sides cut at 16 384 as the operator cuts them
    (w and h themselves stay)."""
    box = np.asarray(box, F)
    w = np.maximum(box[2] - box[0], F(1.0))
    h = np.maximum(box[3] - box[1], F(1.0))
    return w, h, min(int(np.ceil(w)), MAX_SIDE), min(int(np.ceil(h)), MAX_SIDE)


def decode_one(maps, box):
    """maps [S, S, K], box [4] -> (kpt [K, 3], score [K], pos [K]): first arg-max in row-major order (np.argmax: equal floats, -0 == +0, keep the first)."""
    box = np.asarray(box, F)
    w, h, wc, hc = box_sizes(box)
    cw, ch = w / F(wc), h / F(hc)
    K = maps.shape[2]
    kpt, score, pos = np.zeros((K, 3), F), np.zeros(K, F), np.zeros(K, np.int64)
    for k in range(K):
        r = resize_bicubic(maps[:, :, k], hc, wc)
        p = int(np.argmax(r))
        xi, yi = p % wc, p // wc
        kpt[k] = ((F(xi) + F(0.5)) * cw + box[0], (F(yi) + F(0.5)) * ch + box[1], F(1.0))
        score[k] = r.reshape(-1)[p]
        pos[k] = p
    return kpt, score, pos


def decode(heat, boxes, count):
    """heat [N * cap, S, S, K], boxes [N, cap, 4], count [N] -> (kpt [N, cap, K, 3], kscore [N, cap, K]); slots at or beyond count are zero, their maps unread."""
    N, cap = boxes.shape[:2]
    K = heat.shape[3]
    kpt, ks = np.zeros((N, cap, K, 3), F), np.zeros((N, cap, K), F)
    for n in range(N):
        for c in range(int(count[n])):
            kpt[n, c], ks[n, c], _ = decode_one(heat[n * cap + c], boxes[n, c])
    return kpt, ks


def shuffle(x, K):
    """[R, H, W, 4 K] parity-major (channel (2 py + px) K + k) -> [R, 2 H, 2 W, K]"""
    R, H, W, c = x.shape
    assert c == 4 * K
    return np.ascontiguousarray(x.reshape(R, H, W, 2, 2, K).transpose(0, 1, 3, 2, 4, 5).reshape(R, 2 * H, 2 * W, K))


def heatmap(x, K):
    """The predictor's tail: pixel shuffle, then interpolate(scale_factor 2, bilinear, align_corners False) in the oracle's arithmetic."""
    lr = shuffle(np.asarray(x, F), K)
    return ora.resize_bilinear(lr, 2 * lr.shape[1], 2 * lr.shape[2])


def conv_transpose2d_fp64(x, w, b):
    """ConvTranspose2d(kernel 4, stride 2, padding 1) from its definition, in fp64: input pixel (y, x) adds in[y][x][:] . W[:, k, ky, kx] to output pixel
    (2 y - 1 + ky, 2 x - 1 + kx).  x [R, H, W, Cin], w [Cin, K, 4, 4], b [K] -> [R, 2 H, 2 W, K].  (tests/test_keypointrcnn_cpu.py holds it against torch.)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    R, H, W, _ = x.shape
    K = w.shape[1]
    full = np.zeros((R, 2 * H + 2, 2 * W + 2, K), np.float64)      # output coordinates -1 .. 2 H: the padding rows and columns are cut at the end
    for ky in range(4):
        for kx in range(4):
            full[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += x @ w[:, :, ky, kx]
    return full[:, 1:2 * H + 1, 1:2 * W + 1] + np.asarray(b, np.float64)


def roi_features(P, boxes, image_index, aligned=0):
    """RoIAlign 14 x 14 of `boxes` [D, 4] of image `image_index` over P2..P5 ([N, H, W, 256] each), level by level as the mask head's pooler."""
    D = boxes.shape[0]
    out = np.zeros((D, 14, 14, P[0].shape[3]), F)
    lv = ora.level_map(boxes)
    for k in range(2, 6):
        idx = np.nonzero(lv == k)[0]
        if len(idx):
            rois = np.concatenate([np.full((len(idx), 1), image_index, F), boxes[idx]], 1)
            out[idx] = ora.roi_align(P[k - 2], rois, 1.0 / (4 << (k - 2)), 14, 14, 2, aligned)
    return out


def pack_records(box, count, score, label, kpt, kscore, ratios, n_block):
    """The keypoint record block from the engine's whole det.* buffers of the n images of a forward (numpy restatement of pack_keypoint_records_kernel:
    rows past an image's count are copied as they are -- the engine keeps them zero) -> uint8 [total]"""
    from isegmi.dist import coco_record_layout
    n, K = box.shape[:2]
    NK = kpt.shape[2]
    secs, _, total = coco_record_layout(n_block, K, 2, False, 0, box_only=True, keypoints=NK)
    buf = np.zeros(total, np.uint8)
    r = np.asarray(ratios, F).reshape(n, 2)
    vals = dict(box=np.asarray(box, F) * np.concatenate([r, r], 1)[:, None, :], count=count, score=score, label=label,
                kpt=np.asarray(kpt, F) * np.concatenate([r, np.ones((n, 1), F)], 1)[:, None, None, :], kscore=kscore)
    for name, v in vals.items():
        off, nb, dt, shp = secs[name]
        full = np.zeros(shp, dt)
        full[:n] = v
        buf[off:off + nb] = full.view(np.uint8).ravel()
    return buf
