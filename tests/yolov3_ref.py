"""CPU reference of the YOLOv3 forward and its tail (TEST INFRASTRUCTURE ONLY), composed from the oracle's ops: ora.conv2d with act 3 / 4, ora.map_f32 fn 0 / 1,
ora.topk, and -- through tests/retinanet_ref.postprocess -- ora.nms.  It restates DESIGN.md 17 ([UPSTREAM-RECALL] the public yolov3.cfg, unverified).

The keyword forks of select_level / decode_level / YoloV3Ref that are NOT the model (ge_threshold, tie_high_index, best_by_logit, swap_concat, swap_xy) exist for the
discrimination checks of tests/test_yolov3_cpu.py: a crafted input proves its point only if the wrong rule gives another answer on it."""
import numpy as np

import retinanet_ref as rr
from oracle import ora

F32 = np.float32
STRIDES = (32, 16, 8)
ANCHORS = np.asarray([[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]], F32)
WIDTHS = (512, 256, 128)


def sigmoid(x):
    return ora.map_f32(np.asarray(x, F32), 1)


def exp(x):
    return ora.map_f32(np.asarray(x, F32), 0)


def scores(head, A=3, multi_label=True, best_by_logit=False):
    """One (level, image) head [H, W, A*(5+C)] -> the score of every (anchor, class) pair in flat index order [H*W*A*C]; a pair that cannot be a candidate
    (multi_label False: not its anchor's best class) holds -1."""
    rec = np.asarray(head, F32).reshape(-1, A, head.shape[-1] // A).reshape(-1, head.shape[-1] // A)
    obj = sigmoid(rec[:, 4])
    p = sigmoid(rec[:, 5:])
    s = (obj[:, None] * p).astype(F32)   # one rounded fp32 multiply
    if multi_label:
        return s.reshape(-1)
    best = np.argmax(rec[:, 5:] if best_by_logit else p, axis=1)   # argmax: the lowest index of equal values
    out = np.full_like(s, -1)
    r = np.arange(len(rec))
    out[r, best] = s[r, best]
    return out.reshape(-1)


def select_level(head, A=3, top_n=1024, thr=0.5, multi_label=True, ge_threshold=False, tie_high_index=False, best_by_logit=False):
    """-> (scores, flat indices, candidates before the cut) of the min(#candidates, top_n) best, (score desc, index asc)."""
    s = scores(head, A, multi_label, best_by_logit)
    cand = np.flatnonzero(s >= F32(thr) if ge_threshold else s > F32(thr)).astype(np.int64)   # NaN never passes
    if cand.size == 0:
        return np.zeros(0, F32), np.zeros(0, np.int32), 0
    if tie_high_index:
        v, i = ora.topk(s[cand][::-1], top_n)
        return v, cand[::-1][i].astype(np.int32), int(cand.size)
    v, i = ora.topk(s[cand], top_n)   # cand ascends: ora.topk's index order is the flat index order
    return v, cand[i].astype(np.int32), int(cand.size)


def decode_level(sc, idx, head, stride, anchors, canvas_w, canvas_h, A=3, min_wh=0.0, swap_xy=False):
    """The selected of one (level, image) -> (boxes, scores, labels); every operation is its own rounded fp32 operation."""
    H, W, ch = head.shape
    C = ch // A - 5
    idx = np.asarray(idx, np.int64)
    if idx.size == 0:
        return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    rec = idx // C
    cell, a = rec // A, rec % A
    gy, gx = cell // W, cell % W
    if swap_xy:
        gy, gx = cell % H, cell // H
    t = np.asarray(head, F32).reshape(-1, 5 + C)[rec]
    st = F32(stride)
    bx = ((sigmoid(t[:, 0]) + gx.astype(F32)).astype(F32) * st).astype(F32)
    by = ((sigmoid(t[:, 1]) + gy.astype(F32)).astype(F32) * st).astype(F32)
    an = np.asarray(anchors, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hw = ((exp(t[:, 2]) * an[a, 0]).astype(F32) * F32(0.5)).astype(F32)
        hh = ((exp(t[:, 3]) * an[a, 1]).astype(F32) * F32(0.5)).astype(F32)
        b = np.stack([bx - hw, by - hh, bx + hw, by + hh], 1).astype(F32)
        for k, hi in ((0, canvas_w), (1, canvas_h), (2, canvas_w), (3, canvas_h)):
            v = b[:, k]
            b[:, k] = np.where(v < 0, F32(0), np.where(v > F32(hi), F32(hi), v))   # a NaN stays
        ok = ~np.isnan(b).any(1) & ((b[:, 2] - b[:, 0]) >= F32(min_wh)) & ((b[:, 3] - b[:, 1]) >= F32(min_wh))
    return b[ok], np.asarray(sc, F32)[ok], (idx % C + 1).astype(np.int32)[ok]


def select_decode(heads, strides=STRIDES, anchors=ANCHORS, A=3, top_n=1024, thr=0.5, multi_label=True, min_wh=0.0, canvas_w=416, canvas_h=416, **forks):
    """heads[l] [N, H, W, A*(5+C)] -> (dec[l][n] = (boxes, scores, labels), total [N, nl])."""
    N = heads[0].shape[0]
    dkw = {k: forks.pop(k) for k in ("swap_xy",) if k in forks}
    dec, total = [], np.zeros((N, len(heads)), np.int32)
    for l, h in enumerate(heads):
        row = []
        for n in range(N):
            s, i, t = select_level(h[n], A, top_n, thr, multi_label, **forks)
            total[n, l] = t
            row.append(decode_level(s, i, h[n], strides[l], anchors[l], canvas_w, canvas_h, A, min_wh, **dkw))
        dec.append(row)
    return dec, total


def tail(heads, nms_thr=0.4, det_per_img=100, cap=100, nms_flags=2, **kw):
    """-> (dec, total, dets[n] = (boxes, scores, labels)): class-wise NMS with plain areas (flag 2) over the three levels' lists."""
    dec, total = select_decode(heads, **kw)
    C = heads[0].shape[-1] // kw.get("A", 3) - 5
    dets = []
    for n in range(heads[0].shape[0]):
        dets.append(rr.postprocess(np.concatenate([d[n][0] for d in dec]), np.concatenate([d[n][1] for d in dec]), np.concatenate([d[n][2] for d in dec]),
                                   nms_thr, det_per_img, cap, nms_flags, C + 1))
    return dec, total, dets


def concat_up2x(coarse, skip, swap_concat=False):
    up = np.repeat(np.repeat(np.asarray(coarse, F32), 2, axis=1), 2, axis=2)
    return np.ascontiguousarray(np.concatenate([skip, up] if swap_concat else [up, skip], -1))


def _krsc(w):
    return np.ascontiguousarray(np.transpose(np.asarray(w, F32), (0, 2, 3, 1)))


class YoloV3Ref:
    def __init__(self, sd, bn_eps=1e-5, swap_concat=False, **tail_kw):
        self.sd, self.eps, self.swap_concat, self.kw = sd, F32(bn_eps), swap_concat, tail_kw
        self.feats = {}

    def _cbn(self, x, name, bn, stride, pad, act, residual=None):
        sd = self.sd
        w, b = sd[bn + ".weight"].astype(F32), sd[bn + ".bias"].astype(F32)
        m, v = sd[bn + ".running_mean"].astype(F32), sd[bn + ".running_var"].astype(F32)
        sc = (w / np.sqrt(v + self.eps)).astype(F32)
        return ora.conv2d(x, _krsc(sd[name + ".weight"]), stride, pad, sc, (b - m * sc).astype(F32), residual, act)

    def trunk(self, x):
        x = self._cbn(x, "backbone._preconv.0", "backbone._preconv.1", 1, 1, 3)
        outs = []
        for li, nb in enumerate((1, 2, 8, 8, 4)):
            nm = "backbone.layers.%d" % li
            x = self._cbn(x, nm + ".0.0", nm + ".0.1", 2, 1, 3)
            for b in range(1, nb + 1):
                t = self._cbn(x, "%s.%d.conv1" % (nm, b), "%s.%d.bn1" % (nm, b), 1, 0, 3)
                x = self._cbn(t, "%s.%d.conv2" % (nm, b), "%s.%d.bn2" % (nm, b), 1, 1, 4, residual=x)
            outs.append(x)
        return outs[2:]   # strides 8, 16, 32

    def heads(self, images):
        C = self.trunk(np.asarray(images, F32))
        x, out = C[2], []
        for s in range(3):
            for i in range(5):
                x = self._cbn(x, "head.%d.conv%d" % (s, i), "head.%d.bn%d" % (s, i), 1, i & 1, 3)
            branch = x
            t = self._cbn(branch, "head.%d.conv5" % s, "head.%d.bn5" % s, 1, 1, 3)
            out.append(ora.conv2d(t, _krsc(self.sd["head.%d.conv6.weight" % s]), 1, 0, None, self.sd["head.%d.conv6.bias" % s], None, 0))
            if s < 2:
                r = self._cbn(branch, "head.%d.route" % (s + 1), "head.%d.route_bn" % (s + 1), 1, 0, 3)
                x = concat_up2x(r, C[1 - s], self.swap_concat)
        self.feats = dict(C=C, heads=out)
        return out

    def forward(self, images):
        h = self.heads(images)
        H, W = np.asarray(images).shape[1:3]
        dec, total, dets = tail(h, canvas_w=W, canvas_h=H, **self.kw)
        self.feats.update(dec=dec, total=total)
        return [dict(box=d[0], score=d[1], label=d[2]) for d in dets]
