"""Crafted inputs of the YOLOv3 tail kernels (TEST INFRASTRUCTURE ONLY): tests/test_yolo_ops_gpu.py runs them on the device against tests/yolov3_ref.py,
tests/test_yolov3_cpu.py shows with the reference alone that every case reaches the limit or discriminates the rule it is named for.  Everything is
generated from seeds; a case is a dict of yolov3_ref.select_decode's keyword arguments plus `heads`."""
import functools

import numpy as np

F32 = np.float32
SLICE_FLOATS = 8192          # csrc/yolo_ops.hip YOLO_SLICE (the GPU test holds slice_records() to isegmi_op_yolo_slice_records)
GRIDS = ((1, 1), (2, 3), (3, 2))
OFF = F32(-30.0)             # a logit whose sigmoid (9.4e-14) keeps a record or a class far below every threshold used here
ON = F32(30.0)               # a logit whose sigmoid is exactly 1.0 (checked on the CPU)
ANCH = np.asarray([[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]], F32)
STRIDES = (32, 16, 8)


def slice_records(C):
    return SLICE_FLOATS // (5 + C)


def empty_head(N, H, W, A, C):
    """No record passes: objectness and class logits OFF, box parameters 0."""
    h = np.zeros((N, H, W, A, 5 + C), F32)
    h[..., 4:] = OFF
    return h


def case(heads, A=3, strides=None, anchors=None, **kw):
    nl = len(heads)
    d = dict(heads=[np.ascontiguousarray(h.reshape(h.shape[0], h.shape[1], h.shape[2], -1)) for h in heads], A=A,
             strides=tuple(strides or STRIDES[:nl]), anchors=np.asarray(anchors if anchors is not None else ANCH[:nl, :A], F32),
             top_n=1024, thr=0.5, multi_label=True, min_wh=0.0, canvas_w=96, canvas_h=96)
    d.update(kw)
    return d


def fill_candidates(h, n, k, rng, tie_from=None):
    """Make exactly k (anchor, class) pairs of image n candidates at thr 0.5: objectness ON (obj = 1, s = the class sigmoid) on the records that hold them,
    class logits distinct in (0.1, 6) -- or, from rank tie_from on, all equal (an equal-score run) -- at random flat positions; box parameters random."""
    N, H, W, A, REC = h.shape
    C = REC - 5
    flat = np.sort(rng.choice(H * W * A * C, k, replace=False))
    logit = rng.permutation(np.linspace(0.1, 6.0, k).astype(F32))
    if tie_from is not None:
        order = np.argsort(-logit, kind="stable")
        logit[order[tie_from:]] = logit[order[tie_from]] if tie_from < k else logit[order[-1]]
    rec = h[n].reshape(-1, REC)
    rec[flat // C, 4] = ON
    rec[flat // C, 5 + flat % C] = logit
    rec[:, :4] = rng.normal(0, 0.5, (rec.shape[0], 4)).astype(F32)


@functools.lru_cache(None)
def geometry_cases():
    out = {}
    for nl in (1, 3):
        for C in (1, 2, 80):
            for N in (1, 3):
                for g in range(3 if nl == 1 else 1):
                    rng = np.random.default_rng(100 * nl + 10 * C + N + g)
                    grids = [GRIDS[(g + l + (C % 3)) % 3] for l in range(nl)]
                    heads = [rng.normal(0, 2.0, (N, H, W, 3, 5 + C)).astype(F32) for H, W in grids]
                    out["geom_nl%d_C%d_N%d_g%d" % (nl, C, N, g)] = case(heads, thr=0.3)
    return out


TOP_NS = (1, 63, 64, 65, 1024)


def count_plan(top_n):
    """candidates per (level, image) of a count case: 0, 1, top_n - 1, top_n, top_n + 1 and once more top_n + 1."""
    return [[0, 1], [max(top_n - 1, 0), top_n], [top_n + 1, top_n + 1]]


@functools.lru_cache(None)
def count_cases():
    """nl = 3, N = 2, C = 80 on 2x3 / 3x2 / 2x3 grids (1440 pairs a row)."""
    out = {}
    for top_n in TOP_NS:
        for kind in ("distinct", "tie"):
            rng = np.random.default_rng(7000 + top_n + (kind == "tie"))
            heads = [empty_head(2, H, W, 3, 80) for H, W in (GRIDS[1], GRIDS[2], GRIDS[1])]
            for l, row in enumerate(count_plan(top_n)):
                for n, k in enumerate(row):
                    if k:
                        fill_candidates(heads[l], n, k, rng, tie_from=max(k // 2, 0) if kind == "tie" and k > 1 else None)
            out["count_%s_top%d" % (kind, top_n)] = case(heads, top_n=top_n)
    return out


BORDER_ROWS = ("minus1", "exact", "plus1", "two_plus1")


@functools.lru_cache(None)
def slice_cases():
    """A = 1 rows of rs - 1, rs, rs + 1 and 2 rs + 1 anchor records (rs = the kernel's records per slice), candidates in the first and last record and on
    both sides of every slice border; top_n 3 with an equal-score run, so that the cut has to order candidates of different slices."""
    out = {}
    for C in (1, 80):
        rs = slice_records(C)
        for name, nrec in zip(BORDER_ROWS, (rs - 1, rs, rs + 1, 2 * rs + 1)):
            h = empty_head(2, 1, nrec, 1, C)
            recs = sorted({r for r in (0, rs - 2, rs - 1, rs, rs + 1, 2 * rs - 1, 2 * rs, nrec - 1) if 0 <= r < nrec})
            for n in range(2):
                for j, r in enumerate(recs):
                    h[n, 0, r, 0, 4] = ON
                    h[n, 0, r, 0, 5 + (j * 7 + n) % C] = F32(1.0) if n == 0 else F32(0.5 + 0.25 * (j % 3))   # image 0: all equal
                    h[n, 0, r, 0, :4] = F32(0.1 * j)
            out["slice_C%d_%s" % (C, name)] = case([h], A=1, strides=(8,), anchors=np.asarray([[(10, 13)]], F32), top_n=3,
                                                   canvas_w=8 * nrec, canvas_h=8)
    return out


def product_case():
    """One candidate whose product obj * p has a rounding: to = 0.3, class logit 0.7 (C = 2) on a 2x3 grid."""
    h = empty_head(1, 2, 3, 3, 2)
    h[0, 1, 2, 1, 4] = F32(0.3)
    h[0, 1, 2, 1, 6] = F32(0.7)
    return h


@functools.lru_cache(None)
def threshold_cases():
    from yolov3_ref import scores, sigmoid
    out = {}
    h = product_case()
    s = scores(h[0].reshape(2, 3, -1)).max()
    for name, thr in (("pred", np.nextafter(s, F32(0))), ("at", s), ("succ", np.nextafter(s, F32(1)))):
        out["thr_%s_product" % name] = case([h], thr=float(thr))
    # objectness exactly at the threshold and a class sigmoid of exactly 1.0 (logit 88): s == thr, not a candidate; a second record one float above is one
    g = empty_head(1, 2, 3, 3, 2)
    g[0, 0, 1, 0, 4] = F32(0.25); g[0, 0, 1, 0, 5] = F32(88.0)
    obj = sigmoid(np.asarray([0.25], F32))[0]
    out["thr_objectness_at_threshold"] = case([g], thr=float(obj))
    out["thr_objectness_above_threshold"] = case([g], thr=float(np.nextafter(obj, F32(0))))
    # thresholds 0 and 1 on random heads with records at -inf (obj at dm_sigmoid's floor: the product with a class at the floor underflows to 0)
    rng = np.random.default_rng(77)
    r = rng.normal(0, 3.0, (2, 3, 2, 3, 7)).astype(F32)
    r[0, 0, 0, 0, 4:] = -np.inf
    r[1, 2, 1, 2, 4] = -np.inf; r[1, 2, 1, 2, 5] = F32(88.0)
    out["thr_zero"] = case([r], thr=0.0, top_n=1024)
    out["thr_one"] = case([r], thr=1.0)
    floor = sigmoid(np.asarray([-np.inf], F32))[0]   # 4.156e-39: dm_sigmoid never returns less
    out["thr_below_sigmoid_floor"] = case([r], thr=float(np.nextafter(floor, F32(0))))
    return out


@functools.lru_cache(None)
def edge_cases():
    out = {}
    # multi_label 0: logits 30 (class 2) and 40 (class 5) both have sigmoid 1.0 -- the sigmoid rule keeps class 2, a logit rule class 5
    h = empty_head(1, 2, 3, 3, 8)
    h[0, 1, 1, 2, 4] = F32(1.0); h[0, 1, 1, 2, 5:] = F32(-2.0)
    h[0, 1, 1, 2, 5 + 2] = F32(30.0); h[0, 1, 1, 2, 5 + 5] = F32(40.0)
    h[0, 0, 2, 0, 4] = F32(2.0); h[0, 0, 2, 0, 5:] = np.linspace(-1, 2, 8).astype(F32)
    out["best_class_equal_sigmoids"] = case([h], multi_label=False, thr=0.05)
    out["multi_label_same_input"] = case([h], multi_label=True, thr=0.05)
    # decode edges on the stride-8 level, anchor (16, 30): tw = +inf -> full canvas width, kept; tx = NaN -> dropped; tw = 0 at cell x = 1 -> x1 = 4, x2 = 20: a side of exactly 16;
    # tw = -inf -> a side of 0 (kept at min_wh 0); tw = NaN -> dropped
    an = np.asarray([[(16, 30), (16, 30), (16, 30)]], F32)
    g = empty_head(1, 3, 2, 3, 2)
    for (y, x, a), box in (((0, 0, 0), (0, 0, np.inf, 0)), ((1, 1, 1), (np.nan, 0, 0, 0)), ((2, 1, 2), (0, 0, 0, 0)), ((1, 0, 0), (0, 0, -np.inf, 0)), ((0, 1, 1), (0, 0, np.nan, 0))):
        g[0, y, x, a, :4] = np.asarray(box, F32); g[0, y, x, a, 4] = ON; g[0, y, x, a, 5] = F32(1.0 + y + 0.1 * a)
    kw = dict(strides=(8,), anchors=an, canvas_w=64, canvas_h=64)
    out["decode_inf_nan"] = case([g], **kw)
    out["min_wh_equal_side"] = case([g], min_wh=16.0, **kw)
    out["min_wh_one_float_above"] = case([g], min_wh=float(np.nextafter(F32(16.0), F32(17.0))), **kw)
    out["every_box_dropped"] = case([g], min_wh=1.0e9, **kw)
    return out


@functools.lru_cache(None)
def chain_case():
    """Random heads whose boxes overlap: three levels, C = 2, many candidates a class -- select -> class-wise NMS against the reference's final lists."""
    rng = np.random.default_rng(4242)
    heads = []
    for H, W in ((2, 3), (4, 6), (8, 12)):
        h = rng.normal(0, 1.0, (3, H, W, 3, 7)).astype(F32)
        h[..., :2] *= F32(0.5); h[..., 2:4] *= F32(0.2); h[..., 4] += F32(1.0)
        heads.append(h)
    return case(heads, thr=0.3, canvas_w=96, canvas_h=64)


@functools.lru_cache(None)
def all_select_cases():
    out = {}
    for f in (geometry_cases, count_cases, slice_cases, threshold_cases, edge_cases):
        out.update(f())
    return out


def concat_cases():
    return [(N, hc, wc, cc, cs) for N in (1, 2) for hc, wc in GRIDS for cc, cs in ((32, 64), (128, 256))]


# ---- the engine: seeded weights and inputs, the reference forward computed once per canvas and shared by the CPU and GPU tests
ENGINE_SEED = 1234
ENGINE_CANVASES = ((64, 96), (96, 64), (32, 32))
ENGINE_CONF = 0.05


def engine_input(H, W, N=2):
    return np.random.default_rng(1000 + H).uniform(0, 1, (N, H, W, 3)).astype(F32)


@functools.lru_cache(None)
def engine_weights():
    from isegmi.weights import yolov3_state_dict
    return yolov3_state_dict(ENGINE_SEED)


@functools.lru_cache(None)
def engine_reference(H, W):
    """-> (YoloV3Ref after forward (feats: C, heads, dec, total), detections) at conf_thresh 0.05, everything else default."""
    from yolov3_ref import YoloV3Ref
    ref = YoloV3Ref(engine_weights(), thr=ENGINE_CONF)
    return ref, ref.forward(engine_input(H, W))
