"""Seeded generator of a COCO person-keypoint annotation dict and a keypoint result list for the tests of OKS evaluation.

Contents (make_dataset): about 40 images of differing sizes, 0 to 15 persons and 0 to 25 detections each (the cut at maxDets = 20 bites); crowd
gts; gts with num_keypoints == 0 (zeros as keypoints, a box); gts with one visible keypoint; v of 1 and of 2; gts of area 0; gts in each area range
and exactly on 32^2 and 96^2; images with gts and no detection and the reverse; equal scores; detections that are jittered copies of gts at several
noise scales (0 = an exact copy) plus unrelated ones; detections with v = 0 in some slots; detections without a bbox.

No pair of the fixture is NEAR an IoU threshold: a detection whose reference OKS against any gt of its image lies within MARGIN of a threshold
without being equal to it is rejected and redrawn.  Pairs exactly ON a threshold are built so that both sides must agree: the gt has k1 = 2, 4 or 5
visible keypoints, the detection has m of them coincident (e = 0, exp(-0) = 1 exactly) and every other one 10^6 px away (exp underflows to 0), so
the OKS is 1/2, 3/4 or 3/5 -- each one correctly rounded division, and np.linspace(.5, .95, 10) holds exactly those doubles."""
import numpy as np

import oks_ref

MARGIN = 1e-9
THRS = np.linspace(.5, .95, 10)
ON_THRESHOLD = [(2, 1, 0.5), (4, 3, 0.75), (5, 3, 0.6)]     # (k1, coincident keypoints, the OKS)
AREAS = [0.0, 500.0, 1024.0, 3000.0, 9216.0, 20000.0]        # area 0; 'all' only; on 32^2; medium; on 96^2; large


def near_threshold(v):
    return any(v != t and abs(v - t) <= MARGIN for t in THRS)


def _r2(a):
    return [float(v) for v in np.round(np.asarray(a, np.float64), 2)]


def _gt(rng, K, w, h, kind, area):
    """kind: 'plain', 'crowd', 'none' (num_keypoints 0), 'one' (a single visible keypoint), or an int = exactly that many visible keypoints."""
    bw, bh = rng.uniform(12, w * 0.6), rng.uniform(12, h * 0.6)
    bx, by = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
    kp = np.zeros((K, 3))
    kp[:, 0] = np.round(rng.uniform(bx, bx + bw, K), 2); kp[:, 1] = np.round(rng.uniform(by, by + bh, K), 2)
    if kind == "none":
        v = np.zeros(K)
    elif kind == "one":
        v = np.zeros(K); v[rng.integers(0, K)] = rng.integers(1, 3)
    elif isinstance(kind, int):
        kind = min(kind, K)
        v = np.zeros(K); v[rng.choice(K, kind, replace=False)] = rng.integers(1, 3, kind)
    else:
        v = rng.choice([0, 1, 2], K, p=[0.25, 0.3, 0.45])
        if not v.any():
            v[0] = 2
    kp[:, 2] = v
    kp[v == 0, :2] = 0.0                                       # COCO writes zeros for an unlabelled keypoint
    return {"keypoints": _r2(kp.ravel()), "num_keypoints": int((v > 0).sum()), "bbox": _r2([bx, by, bw, bh]),
            "area": float(area if area is not None else np.round(bw * bh * rng.uniform(0.3, 0.8), 2)), "iscrowd": int(kind == "crowd")}


def _det(rng, K, w, h, g, scale, on=None):
    """A detection for gt g: its keypoints jittered by N(0, 1) * scale * sqrt(area) (0: an exact copy); g None: unrelated; on = m: the first m
    visible keypoints coincide, every other keypoint lies 10^6 px away."""
    if g is None:
        kp = np.zeros((K, 3)); kp[:, 0] = rng.uniform(0, w, K); kp[:, 1] = rng.uniform(0, h, K)
    else:
        kp = np.array(g["keypoints"], np.float64).reshape(K, 3).copy()
        if g["num_keypoints"] == 0:                            # a gt without keypoints: in or around its box
            b = g["bbox"]
            f = 0.4 if scale < 0.1 else 4.0
            kp[:, 0] = b[0] + b[2] / 2 + rng.uniform(-1, 1, K) * b[2] * f; kp[:, 1] = b[1] + b[3] / 2 + rng.uniform(-1, 1, K) * b[3] * f
        elif on is not None:
            vis = np.nonzero(kp[:, 2] > 0)[0]
            far = np.ones(K, bool); far[vis[:on]] = False
            kp[far, 0] += 1e6; kp[far, 1] += 1e6
        else:
            kp[:, :2] += rng.normal(0, 1, (K, 2)) * scale * np.sqrt(max(g["area"], 1.0))
    kp[:, 2] = np.where(rng.uniform(size=K) < 0.15, 0, 1)       # the detection's v is never read: some are 0
    return _r2(kp.ravel())


def make_dataset(seed, n_images=40, K=17, sigmas=None):
    """-> (annotation dict, result list).  Every result has `keypoints`; most have a `bbox` too, as this project's json does.
    sigmas: the K sigmas the margin is kept under (default: the first K of COCO's seventeen)."""
    rng = np.random.default_rng(seed)
    var = oks_ref.variances(oks_ref.SIGMAS[:K] if sigmas is None else sigmas)
    assert len(var) == K
    images, anns, results = [], [], []
    special = ["crowd", "none", "one", 2, 4, 5]
    for i in range(n_images):
        w, h = int(rng.integers(90, 640)), int(rng.integers(90, 480))
        iid = 1000 + 3 * i
        images.append({"id": iid, "height": h, "width": w})
        n_gt = 0 if i == 1 else 15 if i == 2 else int(rng.integers(0, 16))
        n_dt = 0 if i == 0 else 25 if i == 2 else int(rng.integers(0, 26))
        if i == 0:
            n_gt = max(n_gt, 3)                                 # image 0: gts and no detection; image 1: detections and no gt
        gts = []
        for j in range(n_gt):
            n = len(anns) + len(gts)
            kind = special[n % 7] if n % 7 < 6 and n % 2 == 0 else "plain"
            area = AREAS[n % 9] if n % 9 < len(AREAS) else None
            g = _gt(rng, K, w, h, kind, area)
            g.update({"id": 1 + n, "image_id": iid, "category_id": 1})
            gts.append(g)
        dets = []
        for j in range(n_dt):
            for attempt in range(100):
                g = gts[int(rng.integers(0, len(gts)))] if gts and rng.uniform() < 0.8 else None
                on = None
                if g is not None and not g["iscrowd"] and rng.uniform() < 0.5:
                    on = next((m for k1, m, _ in ON_THRESHOLD if g["num_keypoints"] == k1), None)
                kp = _det(rng, K, w, h, g, float(rng.choice([0.0, 0.01, 0.03, 0.08, 0.3])), on)
                if not any(near_threshold(oks_ref.oks_pair(kp, q["keypoints"], q["bbox"], q["area"], var)) for q in gts):
                    break
            else:
                raise AssertionError("no detection off the thresholds in 100 draws")
            r = {"image_id": iid, "category_id": 1, "keypoints": kp, "score": float(np.round(rng.uniform(0.05, 1.0), 2 if j % 3 else 1))}
            if j % 5:
                r["bbox"] = oks_ref.extent(kp)[1]
            dets.append(r)
        anns += gts; results += dets
    return {"images": images, "categories": [{"id": 1, "name": "person"}], "annotations": anns}, results


def perfect_results(gt):
    """One detection per gt that can be matched at all (not crowd, some keypoint labelled): the gt's own keypoints."""
    return [{"image_id": a["image_id"], "category_id": a["category_id"], "keypoints": list(a["keypoints"]), "score": 1.0 - 1e-4 * k}
            for k, a in enumerate(gt["annotations"]) if not a["iscrowd"] and a["num_keypoints"] > 0]


def kernel_items(seed, K, n_gt, n_dt):
    """Items for the kernel alone: (kpts [M][K][3], box [M][4], area [M], var [K]), gts first, n_gt >= 1, n_dt >= 1.  Unlabelled gt slots hold NaN
    coordinates.  With more than one gt, gt 0 has no labelled keypoint and gt 1 has area 0.  The first det coincides with the last gt wherever
    that gt is labelled (OKS exactly 1, or the k1 == 0 branch when it is gt 0)."""
    rng = np.random.default_rng(seed)
    M = n_gt + n_dt
    kp = np.zeros((M, K, 3)); kp[:, :, 0] = rng.uniform(0, 300, (M, K)); kp[:, :, 1] = rng.uniform(0, 200, (M, K))
    kp[:, :, 2] = rng.choice([0, 1, 2], (M, K), p=[0.3, 0.3, 0.4])
    box = np.zeros((M, 4)); box[:, :2] = rng.uniform(0, 100, (M, 2)); box[:, 2:] = rng.uniform(10, 120, (M, 2))
    area = rng.uniform(200, 30000, M)
    if n_gt > 1:
        kp[0, :, 2] = 0
        area[1] = 0.0
    for d in range(n_gt, M):                                   # dets near a gt, so that the values spread over (0, 1]
        g = int(rng.integers(0, n_gt))
        near = np.where(kp[g, :, 2:3] > 0, kp[g, :, :2], kp[d, :, :2])
        kp[d, :, :2] = near + rng.normal(0, 1, (K, 2)) * rng.choice([0.0, 0.02, 0.1]) * np.sqrt(area[g])
    kp[n_gt, :, :2] = np.where(kp[n_gt - 1, :, 2:3] > 0, kp[n_gt - 1, :, :2], 7.0)
    un = kp[:n_gt, :, 2] == 0
    kp[:n_gt, :, 0][un] = np.nan; kp[:n_gt, :, 1][un] = np.nan
    var = oks_ref.variances(oks_ref.SIGMAS[:K] if K <= 17 else list(np.linspace(0.02, 0.11, K)))
    return kp, box, area, var
