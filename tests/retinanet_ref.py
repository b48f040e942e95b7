"""CPU reference of the RetinaNet forward and its tail (TEST INFRASTRUCTURE ONLY), composed from the oracle's ops: ora.conv2d with bias and act,
ora.upsample_nearest2x_add, ora.map_f32(x, 1), ora.topk, ora.decode_boxes, ora.nms; the trunk's layers through oracle/maskrcnn_ref.py.  It restates DESIGN.md 12
([UPSTREAM-RECALL] maskrcnn-benchmark: build_resnet_fpn_p3p7_backbone, RetinaNetHead, RetinaNetPostProcessor).

The keyword forks of select_level / postprocess that are NOT the model (ge_threshold, tie_high_index, cross_class) exist for the discrimination checks of
tests/test_retinanet_cpu.py: a crafted input proves its point only if the wrong rule gives another answer on it."""
import numpy as np

from oracle import ora
from oracle.maskrcnn_ref import MaskRCNNRef, cell_anchors_multi, grid_anchors

F32 = np.float32
ANCHOR_SIZES = (32, 64, 128, 256, 512)
ANCHOR_STRIDES = (8, 16, 32, 64, 128)
ASPECT_RATIOS = (0.5, 1.0, 2.0)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def level_sizes(size, octave=2.0, scales_per_octave=3):
    return tuple(size * octave ** (s / float(scales_per_octave)) for s in range(scales_per_octave))


def level_anchors(l, gh, gw):
    """[gh*gw*9, 4]: anchor (y*gw + x)*9 + a, a ratio-major, scale-minor."""
    return grid_anchors(gh, gw, ANCHOR_STRIDES[l], cell_anchors_multi(ANCHOR_STRIDES[l], level_sizes(ANCHOR_SIZES[l]), ASPECT_RATIOS))


def select_level(logits, top_n=1000, thr=0.05, ge_threshold=False, tie_high_index=False):
    """One (level, image): flat logits -> (scores, flat indices) of the min(#candidates, top_n) best sigmoids above thr, (score desc, index asc)."""
    p = ora.map_f32(np.asarray(logits, F32).reshape(-1), 1)
    cand = np.flatnonzero(p >= F32(thr) if ge_threshold else p > F32(thr)).astype(np.int64)
    if cand.size == 0:
        return np.zeros(0, F32), np.zeros(0, np.int32)
    if tie_high_index:
        s, i = ora.topk(p[cand][::-1], top_n)
        return s, cand[::-1][i].astype(np.int32)
    s, i = ora.topk(p[cand], top_n)   # cand ascends: ora.topk's index order is the flat index order
    return s, cand[i].astype(np.int32)


def decode_level(scores, idx, deltas, anchors, im_w, im_h, C=80, min_size=0.0):
    """The selected of one (level, image) -> (boxes, scores, labels): deltas [HWA, 4], anchors [HWA, 4]."""
    a = np.asarray(idx, np.int64) // C
    if a.size == 0:
        return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    b = ora.decode_boxes(np.asarray(anchors, F32)[a], np.asarray(deltas, F32).reshape(-1, 4)[a], BOX_WEIGHTS, float(im_w), float(im_h))
    ok = ((b[:, 2] - b[:, 0] + F32(1)) >= F32(min_size)) & ((b[:, 3] - b[:, 1] + F32(1)) >= F32(min_size))
    return b[ok], np.asarray(scores, F32)[ok], (np.asarray(idx, np.int64) % C + 1).astype(np.int32)[ok]


def postprocess(boxes, scores, labels, nms_thr=0.4, det_per_img=100, cap=128, nms_flags=0, ncls=81, cross_class=False, return_total=False):
    """select_over_all_levels on the concatenated levels of one image.  nms_flags: 1 suppress on >=, 2 plain areas, 4 index order inside a class."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4); scores = np.asarray(scores, F32); labels = np.asarray(labels, np.int32)
    ob, os_, ol = [], [], []
    if cross_class:   # the WRONG rule: one NMS over all classes
        keep = ora.nms(boxes, scores, nms_thr, 0 if nms_flags & 2 else 1, nms_flags & 1)
        alive = np.zeros(len(scores), bool); alive[keep] = True
    for j in range(1, ncls):
        idx = np.flatnonzero(labels == j)
        if idx.size == 0:
            continue
        if cross_class:
            sub = idx[alive[idx]]
            sub = sub[np.lexsort((sub, -scores[sub].astype(np.float64)))]
            keep = np.searchsorted(idx, sub)
        else:
            keep = ora.nms(boxes[idx], scores[idx], nms_thr, 0 if nms_flags & 2 else 1, nms_flags & 1)
        if nms_flags & 4:
            keep = np.sort(keep)
        ob.append(boxes[idx][keep]); os_.append(scores[idx][keep]); ol.append(np.full(len(keep), j, np.int32))
    if not ob:
        out = (np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32))
        return out + (0,) if return_total else out
    b = np.concatenate(ob); s = np.concatenate(os_); lb = np.concatenate(ol)
    total = len(s)
    if det_per_img > 0 and total > det_per_img:
        ts, _ = ora.topk(s, total)
        m = s >= ts[det_per_img - 1]
        b, s, lb = b[m], s[m], lb[m]
    out = (b[:cap], s[:cap], lb[:cap])
    return out + (total,) if return_total else out


def tail(logits, deltas, anchors, image_hw, top_n=1000, thr=0.05, nms_thr=0.4, det_per_img=100, cap=128, nms_flags=0, C=80):
    """logits[l] [N,H,W,A*C], deltas[l] [N,H,W,A*4], anchors[l] -> (sel[l][n] = (scores, idx), dec[l][n] = (boxes, scores, labels), dets[n], totals[n])."""
    N = logits[0].shape[0]
    sel = [[select_level(lg[n], top_n, thr) for n in range(N)] for lg in logits]
    dec = [[decode_level(*sel[l][n], deltas[l][n], anchors[l], image_hw[n][1], image_hw[n][0], C) for n in range(N)] for l in range(len(logits))]
    dets, totals = [], []
    for n in range(N):
        r = postprocess(np.concatenate([d[n][0] for d in dec]), np.concatenate([d[n][1] for d in dec]), np.concatenate([d[n][2] for d in dec]),
                        nms_thr, det_per_img, cap, nms_flags, C + 1, return_total=True)
        dets.append(r[:3]); totals.append(r[3])
    return sel, dec, dets, totals


class RetinaNetRef:
    def __init__(self, sd, depth=50, top_n=1000, thr=0.05, nms_thr=0.4, det_per_img=100, cap=128, nms_flags=0, bn_eps=0.0, num_convs=4):
        self.m = MaskRCNNRef(sd, depth=depth, bn_eps=bn_eps)   # its layer helpers: FrozenBN conv, bias conv
        self.sd, self.depth, self.num_convs = sd, depth, num_convs
        self.kw = dict(top_n=top_n, thr=thr, nms_thr=nms_thr, det_per_img=det_per_img, cap=cap, nms_flags=nms_flags)
        self.feats = {}

    def trunk(self, x):
        m, sd = self.m, self.sd
        x4 = np.concatenate([x, np.zeros(x.shape[:3] + (1,), F32)], -1)
        w1 = np.ascontiguousarray(np.transpose(np.asarray(sd["backbone.body.stem.conv1.weight"], F32), (0, 2, 3, 1)))
        w1 = np.concatenate([w1, np.zeros(w1.shape[:3] + (1,), F32)], -1)
        from oracle.maskrcnn_ref import _frozen_bn
        sc, sh = _frozen_bn(sd, "backbone.body.stem.bn1", m.bn_eps)
        x = ora.maxpool(ora.conv2d(x4, w1, 2, 3, sc, sh, None, 1), 3, 2, 1)
        Cs = []
        for li, nb in enumerate((3, 4, 23 if self.depth == 101 else 6, 3), 1):
            for b in range(nb):
                nm = "backbone.body.layer%d.%d" % (li, b)
                st = 2 if (b == 0 and li > 1) else 1
                idt = m._cbn(x, nm + ".downsample.0", nm + ".downsample.1", st, 0, 0) if b == 0 else x
                t = m._cbn(x, nm + ".conv1", nm + ".bn1", st, 0, 1)
                t = m._cbn(t, nm + ".conv2", nm + ".bn2", 1, 1, 1)
                x = m._cbn(t, nm + ".conv3", nm + ".bn3", 1, 0, 1, residual=idt)
            Cs.append(x)
        return Cs

    def features(self, images):
        """-> [P3, P4, P5, P6, P7]"""
        m = self.m
        Cs = self.trunk(np.asarray(images, F32))
        last = m._cb(Cs[3], "backbone.fpn.fpn_inner4", 1, 0, 0)
        P5 = m._cb(last, "backbone.fpn.fpn_layer4", 1, 1, 0)
        last = ora.upsample_nearest2x_add(last, m._cb(Cs[2], "backbone.fpn.fpn_inner3", 1, 0, 0))
        P4 = m._cb(last, "backbone.fpn.fpn_layer3", 1, 1, 0)
        last = ora.upsample_nearest2x_add(last, m._cb(Cs[1], "backbone.fpn.fpn_inner2", 1, 0, 0))
        P3 = m._cb(last, "backbone.fpn.fpn_layer2", 1, 1, 0)
        P6 = m._cb(Cs[3], "backbone.fpn.top_blocks.p6", 2, 1, 0)
        P7 = m._cb(np.maximum(P6, F32(0)), "backbone.fpn.top_blocks.p7", 2, 1, 0)
        return [P3, P4, P5, P6, P7]

    def heads(self, P):
        m = self.m
        logits, deltas = [], []
        for p in P:
            c = b = p
            for i in range(self.num_convs):
                c = m._cb(c, "rpn.head.cls_tower.%d" % (2 * i), 1, 1, 1)
                b = m._cb(b, "rpn.head.bbox_tower.%d" % (2 * i), 1, 1, 1)
            logits.append(m._cb(c, "rpn.head.cls_logits", 1, 1, 0))
            deltas.append(m._cb(b, "rpn.head.bbox_pred", 1, 1, 0))
        return logits, deltas

    def forward(self, images, image_hw):
        P = self.features(images)
        logits, deltas = self.heads(P)
        anchors = [level_anchors(l, p.shape[1], p.shape[2]) for l, p in enumerate(P)]
        sel, dec, dets, totals = tail(logits, deltas, anchors, image_hw, **self.kw)
        self.feats = dict(P=P, logits=logits, deltas=deltas, anchors=anchors, sel=sel, dec=dec, totals=totals)
        return [dict(box=d[0], score=d[1], label=d[2]) for d in dets]
