"""COCO evaluation: mask / box / keypoint AP and AR of a COCO result list against a COCO annotation file.

The reference's test commands (Pose2Seg test.py --coco, Yolact eval.py, detectron tools/test_net.py) all end in pycocotools' COCOeval.
pycocotools is not available, so COCO.loadRes, COCOeval.evaluate / accumulate / summarize are restated here.  Everything that describes
pycocotools is [UPSTREAM-RECALL -- unverified]: written from memory of its behaviour, not from its source.  The mask / box IoU of every
(detection, ground truth) pair -- under "keypoints" their object keypoint similarity (OKS, COCOeval.computeOks) -- and the greedy matching run
on the GPU (csrc/cocoeval.hip through isegmi._ffi); accumulate and summarize are numpy.

Deliberate deviations from upstream:
  * dtMatches / gtMatches hold 1 + the partner's index inside its (image, category) group, 0 = unmatched.  Upstream stores annotation ids, so
    that a ground truth with id 0 looks unmatched.
  * a detection's area under iou_type "segm" is its mask area even when the record also carries a bbox (upstream's loadRes looks at "bbox" first).
  * a detection's area under iou_type "keypoints" is the extent area of its keypoints even when the record also carries a bbox (same reason).
  * OKS adds its K terms in keypoint-index order (upstream's np.sum pairs them differently); the order is fixed and stated.
  * the headline AP / AR lines use maxDets[-1] (upstream hard-codes 100 and prints -1 when maxDets has no 100).
"""
import json

import numpy as np

from . import coco as _coco

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_RNG_LBL = ["all", "small", "medium", "large"]
KPT_AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
KPT_AREA_RNG_LBL = ["all", "medium", "large"]
KPT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def _kpt_extent(kp):
    """loadRes' keypoint branch: (area, [x0, y0, w, h]) of the extents of the x and y of K * 3 numbers (v is not looked at)."""
    x, y = kp[0::3], kp[1::3]
    x0, x1, y0, y1 = min(x), max(x), min(y), max(y)
    return (x1 - x0) * (y1 - y0), [x0, y0, x1 - x0, y1 - y0]


def _seg_counts(seg, h, w):
    """A COCO `segmentation` field -> (run counts, (h, w)).  Polygons: the union of the parts (rleFrPoly + rleMerge).
    An RLE's counts are taken as they are: non-negative and adding up to h * w, zero-length runs included -- they cover no pixel."""
    if isinstance(seg, dict):
        sh, sw = (int(v) for v in seg["size"])
        c = seg["counts"]
        if isinstance(c, bytes):
            c = c.decode("ascii")
        counts = _coco.rle_from_string(c) if isinstance(c, str) else [int(v) for v in c]
        if sum(counts) != sh * sw or min(counts, default=0) < 0:
            raise ValueError("RLE counts do not add up to its size %dx%d" % (sh, sw))
        return counts, (sh, sw)
    if h is None or w is None:
        raise ValueError("a polygon segmentation needs the image's height and width")
    parts = [_coco.rle_from_polygon(p, h, w) for p in seg]
    return (parts[0] if len(parts) == 1 else _coco.rle_merge(parts, h * w)), (int(h), int(w))


class COCOGt:
    """Index of a COCO annotation file (path or dict): images, categories, annotations with their masks as RLE run counts."""

    def __init__(self, path_or_dict):
        d = path_or_dict
        if not isinstance(d, dict):
            with open(d) as f:
                d = json.load(f)
        self.images = {int(im["id"]): im for im in d.get("images", [])}
        self.cats = {int(c["id"]): c for c in d.get("categories", [])}
        self.anns = []
        for a in d.get("annotations", []):
            iid = int(a["image_id"])
            if iid not in self.images:
                raise ValueError("annotation %r refers to unknown image %r" % (a.get("id"), iid))
            im = self.images[iid]
            r = {"id": a.get("id"), "image_id": iid, "category_id": int(a["category_id"]), "iscrowd": int(a.get("iscrowd", 0)),
                 "ignore": int(a.get("ignore", 0)), "counts": None, "size": None}
            if a.get("segmentation") is not None:
                r["counts"], r["size"] = _seg_counts(a["segmentation"], im.get("height"), im.get("width"))
            if "area" in a:
                r["area"] = float(a["area"])
            elif r["counts"] is not None:
                r["area"] = float(_coco.rle_area(r["counts"]))
            elif "bbox" in a:
                r["area"] = float(a["bbox"][2]) * float(a["bbox"][3])
            else:
                raise ValueError("annotation %r has neither area, segmentation nor bbox" % (a.get("id"),))
            if "bbox" in a:
                r["bbox"] = [float(v) for v in a["bbox"]]
            elif r["counts"] is not None:
                r["bbox"] = _coco.rle_to_bbox(r["counts"], r["size"][0])
            else:
                r["bbox"] = None
            if a.get("keypoints") is not None:
                r["keypoints"] = [float(v) for v in a["keypoints"]]
                r["num_keypoints"] = int(a["num_keypoints"]) if "num_keypoints" in a else sum(1 for v in r["keypoints"][2::3] if v > 0)
            self.anns.append(r)

    def img_ids(self):
        return sorted(self.images)

    def cat_ids(self):
        return sorted(self.cats) if self.cats else sorted({a["category_id"] for a in self.anns})


class COCODt:
    def __init__(self, anns):
        self.anns = anns


def load_results(gt, results_or_path):
    """COCO.loadRes: a result list (or its json) -> COCODt.  Records with a `segmentation` get their mask area and tight box; records with a
    `bbox` keep it; records with `keypoints` keep them with their extent area and box (a record may carry nothing else).  Ids are 1..n in list
    order.  An image id the annotation file does not know raises."""
    res = results_or_path
    if not isinstance(res, (list, tuple)):
        with open(res) as f:
            res = json.load(f)
    out = []
    for k, a in enumerate(res):
        iid = int(a["image_id"])
        if iid not in gt.images:
            raise ValueError("result %d refers to image %r, which is not in the annotation file" % (k, iid))
        im = gt.images[iid]
        r = {"id": k + 1, "image_id": iid, "category_id": int(a["category_id"]), "score": float(a["score"]), "counts": None, "size": None,
             "bbox": [float(v) for v in a["bbox"]] if a.get("bbox") is not None else None}
        if a.get("segmentation") is not None:
            r["counts"], r["size"] = _seg_counts(a["segmentation"], im.get("height"), im.get("width"))
            r["seg_area"] = float(_coco.rle_area(r["counts"]))
            r["seg_bbox"] = _coco.rle_to_bbox(r["counts"], r["size"][0])
        if a.get("keypoints") is not None:
            r["keypoints"] = [float(v) for v in a["keypoints"]]
            if len(r["keypoints"]) >= 3 and len(r["keypoints"]) % 3 == 0:
                r["kp_area"], r["kp_bbox"] = _kpt_extent(r["keypoints"])
            elif r["counts"] is None and r["bbox"] is None:
                raise ValueError("result %d: keypoints must be K * 3 numbers, got %d" % (k, len(r["keypoints"])))
        if r["counts"] is None and r["bbox"] is None and "keypoints" not in r:
            raise ValueError("result %d has neither bbox, segmentation nor keypoints" % k)
        out.append(r)
    return COCODt(out)


class Params:
    """COCOeval parameters with upstream's defaults for `segm` / `bbox`."""

    def __init__(self, iou_type="segm"):
        if iou_type not in ("segm", "bbox"):
            raise ValueError("iou_type %r: Params covers segm and bbox; keypoints have their own defaults in KeypointParams" % (iou_type,))
        self._defaults(iou_type)

    def _defaults(self, iou_type):
        self.iouType = iou_type
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [list(r) for r in AREA_RNG]
        self.areaRngLbl = list(AREA_RNG_LBL)
        self.useCats = 1


class KeypointParams(Params):
    """[UPSTREAM-RECALL -- unverified] upstream's defaults for `keypoints`: at most 20 detections per image, no `small` range, the per-keypoint
    sigmas of the 17 COCO person keypoints.  K = len(kpt_oks_sigmas); other sigmas (1 to 32 of them) may be set."""

    def __init__(self):
        self._defaults("keypoints")
        self.maxDets = [20]
        self.areaRng = [list(r) for r in KPT_AREA_RNG]
        self.areaRngLbl = list(KPT_AREA_RNG_LBL)
        self.kpt_oks_sigmas = KPT_OKS_SIGMAS.copy()


class COCOeval:
    """evaluate() -> accumulate() -> summarize(), as pycocotools' class of the same name.
    mem_budget: bytes of device memory one chunk of groups may take for its pair list, IoU blocks and match arrays."""

    def __init__(self, gt, dt, iou_type="segm", mem_budget=512 << 20):
        self.gt = gt if isinstance(gt, COCOGt) else COCOGt(gt)
        self.dt = dt if isinstance(dt, COCODt) else load_results(self.gt, dt)
        self.params = KeypointParams() if iou_type == "keypoints" else Params(iou_type)
        self.params.imgIds = self.gt.img_ids()
        self.params.catIds = self.gt.cat_ids()
        self.mem_budget = int(mem_budget)
        self.evalImgs = {}
        self.eval = {}
        self.stats = None
        self.timings = {}

    # ------------------------------------------------------------------------------------------------------------ evaluate
    def _prepare(self):
        p = self.params
        p.imgIds = sorted(set(int(i) for i in p.imgIds))
        p.catIds = sorted(set(int(c) for c in p.catIds)) if p.useCats else [-1]
        p.maxDets = sorted(int(m) for m in p.maxDets)
        segm = p.iouType == "segm"
        kpt = p.iouType == "keypoints"
        if kpt:
            K = len(p.kpt_oks_sigmas)
            if not 1 <= K <= 32:
                raise ValueError("kpt_oks_sigmas: %d sigmas, the OKS kernel takes 1 to 32" % K)
        img_pos = {i: k for k, i in enumerate(p.imgIds)}
        cat_pos = {c: k for k, c in enumerate(p.catIds)}
        groups = {}   # (k, i) -> ([gt ann indices], [dt ann indices])
        for n, a in enumerate(self.gt.anns):
            i = img_pos.get(a["image_id"])
            k = cat_pos.get(a["category_id"]) if p.useCats else 0
            if i is None or k is None:
                continue
            if segm and a["counts"] is None:
                raise ValueError("ground truth %r has no segmentation" % (a["id"],))
            if not segm and a["bbox"] is None:
                raise ValueError("ground truth %r has no bbox" % (a["id"],))
            if kpt and a.get("keypoints") is None:
                raise ValueError("ground truth %r has no keypoints" % (a["id"],))
            if kpt and len(a["keypoints"]) != 3 * K:
                raise ValueError("ground truth %r has %d keypoint numbers, %d sigmas need %d" % (a["id"], len(a["keypoints"]), K, 3 * K))
            groups.setdefault((k, i), ([], []))[0].append(n)
        for n, a in enumerate(self.dt.anns):
            i = img_pos.get(a["image_id"])
            k = cat_pos.get(a["category_id"]) if p.useCats else 0
            if i is None or k is None:
                continue
            if segm and a["counts"] is None:
                raise ValueError("detection %d has no segmentation" % a["id"])
            if kpt and a.get("keypoints") is None:
                raise ValueError("detection %d has no keypoints" % a["id"])
            if kpt and len(a["keypoints"]) != 3 * K:
                raise ValueError("detection %d has %d keypoint numbers, %d sigmas need %d" % (a["id"], len(a["keypoints"]), K, 3 * K))
            groups.setdefault((k, i), ([], []))[1].append(n)
        return groups

    def evaluate(self):
        import time

        from . import _ffi
        p = self.params
        t0 = time.perf_counter()
        groups = self._prepare()
        segm = p.iouType == "segm"
        kpt = p.iouType == "keypoints"
        ga, da = self.gt.anns, self.dt.anns
        n_gt_all = len(ga)
        if segm:
            d_area_all = np.array([a.get("seg_area", 0.0) for a in da], np.float64)
        elif kpt:
            d_area_all = np.array([a.get("kp_area", 0.0) for a in da], np.float64)
        else:
            for a in da:
                if a["bbox"] is None:
                    a["bbox"] = a["seg_bbox"] if "seg_bbox" in a else a["kp_bbox"]
            d_area_all = np.array([a["bbox"][2] * a["bbox"][3] for a in da], np.float64)
        d_score_all = np.array([a["score"] for a in da], np.float64)
        g_area_all = np.array([a["area"] for a in ga], np.float64)
        g_crowd_all = np.array([a["iscrowd"] != 0 for a in ga], np.uint8)
        g_ign_all = np.array([a["ignore"] != 0 or (kpt and a.get("num_keypoints", 1) == 0) for a in ga], np.uint8)
        keys = sorted(groups)
        max_det = p.maxDets[-1]
        # per group: gts in annotation order, dets by descending score (stable), cut to maxDets[-1]
        g_lists, d_lists = [], []
        for key in keys:
            gi, di = groups[key]
            di = np.asarray(di, np.int64)
            if di.size:
                di = di[np.argsort(-d_score_all[di], kind="mergesort")][:max_det]
            g_lists.append(np.asarray(gi, np.int64)); d_lists.append(di)
            if segm and len(gi) and di.size:
                sz = ga[gi[0]]["size"]
                for n in di:
                    if da[n]["size"] != sz:
                        raise ValueError("detection %d is %r, its image's ground truth is %r" % (da[n]["id"], da[n]["size"], sz))
        t1 = time.perf_counter()
        # ---- upload every mask / box / keypoint set once
        if segm:
            used_g = [n for n in range(n_gt_all) if ga[n]["counts"] is not None]
            slot_g = np.full(n_gt_all, -1, np.int64); slot_g[used_g] = np.arange(len(used_g))
            rles = _ffi.RleSet([ga[n]["counts"] for n in used_g] + [a["counts"] for a in da],
                               [ga[n]["size"] for n in used_g] + [a["size"] for a in da])
            slot_d = len(used_g) + np.arange(len(da), dtype=np.int64)
            n_items = rles.M
        elif kpt:
            # one item list, gts first: a gt brings keypoints, box and area; of a det only the keypoints are read
            K = len(p.kpt_oks_sigmas)
            used_g = [n for n in range(n_gt_all) if ga[n].get("keypoints") is not None and len(ga[n]["keypoints"]) == 3 * K
                      and ga[n]["bbox"] is not None]
            used_d = [n for n in range(len(da)) if da[n].get("keypoints") is not None and len(da[n]["keypoints"]) == 3 * K]
            slot_g = np.full(n_gt_all, -1, np.int64); slot_g[used_g] = np.arange(len(used_g))
            slot_d = np.full(len(da), -1, np.int64); slot_d[used_d] = len(used_g) + np.arange(len(used_d))
            n_items = len(used_g) + len(used_d)
            kp = np.array([ga[n]["keypoints"] for n in used_g] + [da[n]["keypoints"] for n in used_d], np.float64).reshape(n_items, K, 3)
            kbox = np.zeros((n_items, 4), np.float64); karea = np.zeros(n_items, np.float64)
            kbox[:len(used_g)] = np.array([ga[n]["bbox"] for n in used_g], np.float64).reshape(-1, 4)
            karea[:len(used_g)] = g_area_all[used_g]
            sig = np.asarray(p.kpt_oks_sigmas, np.float64)
            d_kp = [_ffi.DeviceBuffer.from_numpy(a) for a in (kp, kbox, karea, (sig * 2) ** 2)]
        else:
            used_g = [n for n in range(n_gt_all) if ga[n]["bbox"] is not None]
            slot_g = np.full(n_gt_all, -1, np.int64); slot_g[used_g] = np.arange(len(used_g))
            boxes = np.array([ga[n]["bbox"] for n in used_g] + [a["bbox"] for a in da], np.float64).reshape(-1, 4)
            d_boxes = _ffi.DeviceBuffer.from_numpy(boxes)
            slot_d = len(used_g) + np.arange(len(da), dtype=np.int64)
            n_items = len(boxes)
        _ffi.sync()
        t2 = time.perf_counter() - (rles.prefix_seconds if segm else 0.0)
        A, T = len(p.areaRng), len(p.iouThrs)
        Dn = np.array([len(d) for d in d_lists], np.int64); Gn = np.array([len(g) for g in g_lists], np.int64)
        # per pair 12 bytes of pair list and 8 of IoU / OKS; the items (RLEs, boxes, keypoint sets) are uploaded once, outside the chunks
        cost = Dn * Gn * 20 + A * T * (Dn * 5 + Gn * 4) + A * Gn + 64
        self.evalImgs = {}
        self.timings = {"prepare": t1 - t0, "upload": t2 - t1, "prefix": rles.prefix_seconds if segm else 0.0, "iou": 0.0, "match": 0.0,
                        "chunks": 0, "pairs": 0, "groups": len(keys)}
        lo = 0
        while lo < len(keys):
            hi, acc = lo, 0
            while hi < len(keys) and (hi == lo or acc + cost[hi] <= self.mem_budget):
                acc += int(cost[hi]); hi += 1
            D, G = Dn[lo:hi], Gn[lo:hi]
            det_off = np.zeros(hi - lo + 1, np.int64); np.cumsum(D, out=det_off[1:])
            gt_off = np.zeros(hi - lo + 1, np.int64); np.cumsum(G, out=gt_off[1:])
            iou_off = np.zeros(hi - lo + 1, np.int64); np.cumsum(D * G, out=iou_off[1:])
            dets = np.concatenate(d_lists[lo:hi]) if det_off[-1] else np.zeros(0, np.int64)
            gts = np.concatenate(g_lists[lo:hi]) if gt_off[-1] else np.zeros(0, np.int64)
            P = int(iou_off[-1])
            grp = np.repeat(np.arange(hi - lo), D * G)
            local = np.arange(P, dtype=np.int64) - iou_off[grp]
            gw = G[grp]
            dl, gl = local // np.maximum(gw, 1), local % np.maximum(gw, 1)
            pairs = np.empty((P, 3), np.int32)
            gsel = gts[gt_off[grp] + gl] if P else np.zeros(0, np.int64)
            pairs[:, 0] = slot_d[dets[det_off[grp] + dl]] if P else 0
            pairs[:, 1] = slot_g[gsel] if P else 0
            pairs[:, 2] = g_crowd_all[gsel] if P else 0
            tc0 = time.perf_counter()
            d_pairs = _ffi.DeviceBuffer.from_numpy(pairs); d_ious = _ffi.DeviceBuffer((max(P, 1),), np.float64)
            if segm:
                _ffi.rle_iou_device(rles, d_pairs, P, d_ious)
            elif kpt:
                _ffi.oks_device(*d_kp, n_items, K, d_pairs, P, d_ious)
            else:
                _ffi.bbox_iou_device(d_boxes, n_items, d_pairs, P, d_ious)
            _ffi.sync()
            tc1 = time.perf_counter()
            dtm, dti, gtm, gti = _ffi.coco_match(det_off, gt_off, iou_off[:-1], None, d_area_all[dets], g_area_all[gts], g_crowd_all[gts],
                                                 g_ign_all[gts], p.areaRng, p.iouThrs, d_ious=d_ious)
            tc2 = time.perf_counter()
            ious = d_ious.numpy()[:P]
            if P and (ious < 0).any():
                raise _ffi.IsegmiError("the IoU kernel rejected a pair (index or size mismatch)")
            d_pairs.free(); d_ious.free()
            self.timings["iou"] += tc1 - tc0; self.timings["match"] += tc2 - tc1; self.timings["chunks"] += 1
            self.timings["pairs"] += P
            for j in range(hi - lo):
                d0, d1, g0, g1 = det_off[j], det_off[j + 1], gt_off[j], gt_off[j + 1]
                self.evalImgs[keys[lo + j]] = {
                    "dtIds": [da[n]["id"] for n in dets[d0:d1]], "gtIds": [ga[n]["id"] for n in gts[g0:g1]],
                    "dtScores": d_score_all[dets[d0:d1]], "dtMatches": dtm[:, :, d0:d1], "dtIgnore": dti[:, :, d0:d1],
                    "gtMatches": gtm[:, :, g0:g1], "gtIgnore": gti[:, g0:g1],
                    "ious": ious[iou_off[j]:iou_off[j + 1]].reshape(int(D[j]), int(G[j]))}
            lo = hi
        if segm:
            rles.free()
        elif kpt:
            for b in d_kp:
                b.free()
        else:
            d_boxes.free()
        self.timings["total"] = time.perf_counter() - t0
        return self.evalImgs

    # ------------------------------------------------------------------------------------------------------------ accumulate
    def accumulate(self):
        """Host numpy.  precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M]; -1 where a cell has no non-ignored gt."""
        self.eval = accumulate(self.evalImgs, self.params)
        return self.eval

    def summarize(self):
        self.stats, lines = summarize(self.eval, self.params)
        return lines


def accumulate(eval_imgs, p):
    """eval_imgs: {(category index, image index): {"dtScores" [D], "dtMatches" [A, T, D], "dtIgnore" [A, T, D], "gtIgnore" [A, G]}} with the
    detections of a group in descending score order.  [UPSTREAM-RECALL -- unverified] COCOeval.accumulate."""
    T, R, A, M = len(p.iouThrs), len(p.recThrs), len(p.areaRng), len(p.maxDets)
    K = len(p.catIds) if p.useCats else 1
    precision = -np.ones((T, R, K, A, M)); recall = -np.ones((T, K, A, M)); scores = -np.ones((T, R, K, A, M))
    rec_thrs = np.asarray(p.recThrs, np.float64)
    by_cat = {}
    for (k, i) in sorted(eval_imgs):
        by_cat.setdefault(k, []).append(eval_imgs[(k, i)])
    for k, E in by_cat.items():
        for a in range(A):
            gt_ig = np.concatenate([e["gtIgnore"][a] for e in E])
            npig = int(np.count_nonzero(gt_ig == 0))
            if npig == 0:
                continue
            for m, max_det in enumerate(p.maxDets):
                sc = np.concatenate([e["dtScores"][:max_det] for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                sc_sorted = sc[inds]
                dtm = np.concatenate([e["dtMatches"][a][:, :max_det] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["dtIgnore"][a][:, :max_det] for e in E], axis=1)[:, inds]
                tps = np.logical_and(dtm != 0, dtig == 0)
                fps = np.logical_and(dtm == 0, dtig == 0)
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros(R); ss = np.zeros(R)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                        at = np.searchsorted(rc, rec_thrs, side="left")
                        ok = at < nd
                        q[ok] = pr[at[ok]]
                        ss[ok] = sc_sorted[at[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return {"counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}


def summarize(ev, p):
    """-> (stats [12], the twelve lines in upstream's format); under `keypoints` stats [10] and ten lines, all at maxDets[-1] (20)."""
    lines = []

    def one(ap, iou_thr=None, area="all", max_dets=None):
        max_dets = p.maxDets[-1] if max_dets is None else max_dets
        a = [i for i, l in enumerate(p.areaRngLbl) if l == area]
        m = [i for i, v in enumerate(p.maxDets) if v == max_dets]
        s = ev["precision"] if ap else ev["recall"]
        if iou_thr is not None:
            s = s[np.where(np.isclose(np.asarray(p.iouThrs), iou_thr, rtol=0, atol=1e-9))[0]]
        s = s[..., a, m] if ap else s[:, :, a, m]
        v = s[s > -1]
        mean = -1.0 if v.size == 0 else float(np.mean(v))
        iou_s = "{:0.2f}:{:0.2f}".format(p.iouThrs[0], p.iouThrs[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_s, area, max_dets, mean))
        return mean
    md = p.maxDets
    if p.iouType == "keypoints":
        stats = np.zeros(10)
        for ap in (1, 0):
            o = 0 if ap else 5
            stats[o + 0] = one(ap, max_dets=md[-1])
            stats[o + 1] = one(ap, iou_thr=.5, max_dets=md[-1])
            stats[o + 2] = one(ap, iou_thr=.75, max_dets=md[-1])
            stats[o + 3] = one(ap, area="medium", max_dets=md[-1])
            stats[o + 4] = one(ap, area="large", max_dets=md[-1])
        return stats, lines
    stats = np.zeros(12)
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5, max_dets=md[-1])
    stats[2] = one(1, iou_thr=.75, max_dets=md[-1])
    stats[3] = one(1, area="small", max_dets=md[-1])
    stats[4] = one(1, area="medium", max_dets=md[-1])
    stats[5] = one(1, area="large", max_dets=md[-1])
    stats[6] = one(0, max_dets=md[0])
    stats[7] = one(0, max_dets=md[min(1, len(md) - 1)])
    stats[8] = one(0, max_dets=md[-1])
    stats[9] = one(0, area="small", max_dets=md[-1])
    stats[10] = one(0, area="medium", max_dets=md[-1])
    stats[11] = one(0, area="large", max_dets=md[-1])
    return stats, lines


def evaluate_results(gt, results, iou_types=("bbox", "segm"), cat_ids=None, max_dets=None, verbose=False, mem_budget=512 << 20):
    """One call from a result list (or json path) to {iou_type: stats [12]} ([10] for "keypoints")."""
    gt = gt if isinstance(gt, COCOGt) else COCOGt(gt)
    dt = results if isinstance(results, COCODt) else load_results(gt, results)
    out = {}
    for it in iou_types:
        e = COCOeval(gt, dt, it, mem_budget=mem_budget)
        if cat_ids:
            e.params.catIds = list(cat_ids)
        if max_dets:
            e.params.maxDets = list(max_dets)
        e.evaluate()
        e.accumulate()
        lines = e.summarize()
        if verbose:
            print("COCO %s evaluation:" % it)
            print("\n".join(lines))
        out[it] = e.stats
    return out
