"""RetinaNet without a GPU: the config mapping and its refusals, the anchors, a torch restatement of the two post-processor functions against
tests/retinanet_ref.py, the proof that every crafted op input of tests/retinanet_cases.py discriminates the rule or reaches the limit it is named for, and
the weights."""
import os
import sys

import numpy as np
import pytest

import retinanet_cases as rc
import retinanet_ref as rr
from oracle import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
YAML = os.path.join(ROOT, "configs", "retinanet_R-%d-FPN_1x.yaml")


def _node(depth=50, *kv):
    from isegmi.config import cfg
    c = cfg.clone()
    c.merge_from_file(YAML % depth)
    c.merge_from_list(list(kv))
    return c


# ------------------------------------------------------------------------------------------------------------------- config
def test_yaml_maps_to_retinanet_config():
    from isegmi.config import is_retinanet, to_retinanet_config
    from isegmi.retinanet import RetinaNetConfig
    for depth in (50, 101):
        c = _node(depth)
        assert is_retinanet(c)
        rc_ = to_retinanet_config(c)
        assert rc_ == RetinaNetConfig(depth=depth, CONV_BODY="R-%d-FPN-RETINANET" % depth)
        assert (rc_.PRE_NMS_TOP_N, rc_.INFERENCE_TH, rc_.NMS_TH, rc_.DETECTIONS_PER_IMG, rc_.NUM_CONVS) == (1000, 0.05, 0.4, 100, 4)
        assert rc_.ANCHOR_STRIDES == (8, 16, 32, 64, 128) and rc_.det_cap == 100
    rc_ = to_retinanet_config(_node(50, "MODEL.RETINANET.PRE_NMS_TOP_N", 500, "MODEL.RETINANET.NMS_TH", 0.5, "TEST.DETECTIONS_PER_IMG", 50))
    assert (rc_.PRE_NMS_TOP_N, rc_.NMS_TH, rc_.DETECTIONS_PER_IMG) == (500, 0.5, 50)


@pytest.mark.parametrize("kv, key", [
    (("MODEL.RETINANET.USE_C5", False), "MODEL.RETINANET.USE_C5"),
    (("MODEL.RETINANET.NUM_CONVS", 0), "MODEL.RETINANET.NUM_CONVS"),
    (("MODEL.FPN.USE_GN", True), "MODEL.FPN.USE_GN"),
    (("MODEL.RESNETS.TRANS_FUNC", "BottleneckWithGN"), "MODEL.RESNETS.TRANS_FUNC"),
    (("MODEL.RESNETS.STEM_FUNC", "StemWithGN"), "MODEL.RESNETS.STEM_FUNC"),
    (("MODEL.BACKBONE.CONV_BODY", "R-50-FPN"), "MODEL.BACKBONE.CONV_BODY"),
    (("MODEL.BACKBONE.CONV_BODY", "R-152-FPN-RETINANET"), "MODEL.BACKBONE.CONV_BODY"),
    (("MODEL.RETINANET.NUM_CLASSES", 21), "MODEL.RETINANET.NUM_CLASSES"),
    (("MODEL.MASK_ON", True), "MODEL.MASK_ON"),
    (("MODEL.RETINANET.PRE_NMS_TOP_N", 2000), "MODEL.RETINANET.PRE_NMS_TOP_N"),
    (("MODEL.RETINANET.ANCHOR_STRIDES", "(8, 16, 32, 64)"), "MODEL.RETINANET.ANCHOR_STRIDES"),
    (("MODEL.RETINANET_ON", False), "MODEL.RETINANET_ON"),
])
def test_every_refusal_names_its_key(kv, key):
    from isegmi.config import to_retinanet_config
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        to_retinanet_config(_node(50, *kv))


def test_maskrcnn_mapping_is_unchanged():
    from isegmi.config import cfg, to_maskrcnn_config
    with pytest.raises(ValueError, match="built bodies"):
        to_maskrcnn_config(_node(50))
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_mask_rcnn_R_50_FPN_1x.yaml"))
    from isegmi.maskrcnn import MaskRCNNConfig
    assert to_maskrcnn_config(c) == MaskRCNNConfig()
    assert cfg.MODEL.RETINANET_ON is False and cfg.TEST.DETECTIONS_PER_IMG == 100


# ------------------------------------------------------------------------------------------------------------------- anchors
def test_anchors():
    from isegmi.maskrcnn import generate_anchors_multi, grid_anchors
    from isegmi.retinanet import RetinaNetConfig, retina_level_shapes
    cfg = RetinaNetConfig()
    assert cfg.level_sizes(32) == (32.0, 32 * 2 ** (1 / 3.0), 32 * 2 ** (2 / 3.0))
    assert cfg.level_sizes(512)[2] == 512 * 2.0 ** (2 / 3.0)
    assert rr.level_sizes(64) == cfg.level_sizes(64)
    base = generate_anchors_multi(8, cfg.level_sizes(32), cfg.ASPECT_RATIOS)
    assert base.shape == (9, 4)
    assert base[0].tolist() == [-18.0, -8.0, 25.0, 15.0]     # hand-derived: stride 8, ratio 0.5, size 32
    ws, hs = base[:, 2] - base[:, 0] + 1, base[:, 3] - base[:, 1] + 1
    assert np.all(np.diff(ws[:3]) > 0) and np.all(np.diff(ws[3:6]) > 0)           # scale-minor inside a ratio
    assert np.all(hs[:3] < ws[:3]) and np.all(hs[6:] > ws[6:]) and np.allclose(hs[3:6], ws[3:6])   # ratio-major: 0.5, 1, 2
    shapes = retina_level_shapes(256, 352)
    assert shapes == [(32, 44), (16, 22), (8, 11), (4, 6), (2, 3)] and retina_level_shapes(128, 160)[4] == (1, 2)
    assert retina_level_shapes(800, 1344)[0] == (100, 168)
    for l, (h, w) in enumerate(shapes):
        a = rr.level_anchors(l, h, w)
        assert a.shape == (h * w * 9, 4)
        b = grid_anchors(h, w, cfg.ANCHOR_STRIDES[l], generate_anchors_multi(cfg.ANCHOR_STRIDES[l], cfg.level_sizes(cfg.ANCHOR_SIZES[l]), cfg.ASPECT_RATIOS))
        assert np.array_equal(a, b)
        assert np.array_equal(a[9 + 4] - a[4], np.full(4, 0, F32) + [cfg.ANCHOR_STRIDES[l], 0, cfg.ANCHOR_STRIDES[l], 0])


# ------------------------------------------------------------------------------------------------------------------- second opinion
def _torch_single_feature_map(logits, deltas, anchors, im_w, im_h, top_n, thr, C):
    """forward_for_single_feature_map, restated in torch from DESIGN.md 12 (one image)."""
    import torch
    p = torch.from_numpy(ora.map_f32(logits.reshape(-1), 1))      # the engine's sigmoid; everything after it is torch
    cand = torch.nonzero(p > thr).flatten()
    k = min(int(cand.numel()), top_n)
    s, order = torch.topk(p[cand], k, sorted=True)
    idx = cand[order]
    a = torch.from_numpy(anchors)[idx // C]
    d = torch.from_numpy(deltas.reshape(-1, 4))[idx // C]
    w = a[:, 2] - a[:, 0] + 1; h = a[:, 3] - a[:, 1] + 1
    cx = a[:, 0] + 0.5 * w; cy = a[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / 10, d[:, 1] / 10
    dw = torch.clamp(d[:, 2] / 5, max=float(np.log(1000.0 / 16))); dh = torch.clamp(d[:, 3] / 5, max=float(np.log(1000.0 / 16)))
    pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    b = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, im_w - 1); b[:, 1::2] = b[:, 1::2].clamp(0, im_h - 1)
    return b, s, idx % C + 1


def _torch_select_over_all_levels(b, s, lb, nms_thr, det):
    import torch

    def nms(boxes, scores):
        order = torch.argsort(scores, descending=True, stable=True).tolist()
        keep = []
        area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        dead = set()
        for n_, i in enumerate(order):
            if i in dead:
                continue
            keep.append(i)
            for j in order[n_ + 1:]:
                if j in dead:
                    continue
                iw = (torch.min(boxes[i, 2], boxes[j, 2]) - torch.max(boxes[i, 0], boxes[j, 0]) + 1).clamp(min=0)
                ih = (torch.min(boxes[i, 3], boxes[j, 3]) - torch.max(boxes[i, 1], boxes[j, 1]) + 1).clamp(min=0)
                inter = iw * ih
                if inter / (area[i] + area[j] - inter) > nms_thr:
                    dead.add(j)
        return keep
    ob, os_, ol = [], [], []
    for j in range(1, 81):
        idx = torch.nonzero(lb == j).flatten()
        if idx.numel() == 0:
            continue
        keep = nms(b[idx], s[idx])
        ob.append(b[idx][keep]); os_.append(s[idx][keep]); ol.append(torch.full((len(keep),), j))
    b, s, lb = torch.cat(ob), torch.cat(os_), torch.cat(ol)
    if len(s) > det:
        kth = torch.kthvalue(s, len(s) - det + 1).values
        m = s >= kth
        b, s, lb = b[m], s[m], lb[m]
    return b, s, lb


def test_second_opinion_in_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(50)
    shapes = ((6, 7), (3, 4))
    A, C, top_n, det = 9, 80, 60, 25
    logits = [rng.uniform(-4.2, -1.0, (1, h, w, A * C)).astype(F32) for h, w in shapes]
    deltas = [(rng.standard_normal((1, h, w, A * 4)) * 2.0).astype(F32) for h, w in shapes]
    anchors = [rr.level_anchors(l, h, w) for l, (h, w) in enumerate(shapes)]
    hw = np.array([[45, 52]], np.int32)
    sel, dec, dets, totals = rr.tail(logits, deltas, anchors, hw, top_n=top_n, det_per_img=det, cap=det)
    for lv in sel:
        assert len(np.unique(lv[0][0])) == len(lv[0][0]) == top_n, "inputs without score ties"
    assert totals[0] > det
    tb, ts, tl = [], [], []
    for l in range(2):
        b, s, lb = _torch_single_feature_map(logits[l][0], deltas[l][0], anchors[l], 52.0, 45.0, top_n, 0.05, C)
        assert np.array_equal(s.numpy(), dec[l][0][1]) and np.array_equal(lb.numpy(), dec[l][0][2])
        assert np.allclose(b.numpy(), dec[l][0][0], rtol=0, atol=2e-3)    # torch.exp against the engine's deterministic exp, boxes up to 52 wide
        tb.append(torch.from_numpy(dec[l][0][0])); ts.append(s); tl.append(lb)
    b, s, lb = _torch_select_over_all_levels(torch.cat(tb), torch.cat(ts), torch.cat(tl), 0.4, det)
    assert len(s) == len(dets[0][1]) == det
    assert np.array_equal(lb.numpy(), dets[0][2]) and np.array_equal(s.numpy(), dets[0][1]) and np.array_equal(b.numpy(), dets[0][0])


# ------------------------------------------------------------------------------------------------------------------- discrimination
def _sel_all(case, **kw):
    logits, a, c, top_n = case
    return [tuple(x.tolist() for x in rr.select_level(lg[n], top_n, 0.05, **kw)) for lg in logits for n in range(lg.shape[0])]


def test_threshold_case_discriminates_strictness():
    x_at, x_up, exact = rc.threshold_logits()
    p = ora.map_f32(np.array([x_at, x_up], F32), 1)
    assert p[0] <= F32(0.05) < p[1] and np.nextafter(x_at, F32(np.inf), dtype=F32) == x_up
    case = rc.select_cases()["threshold_edge"]
    if exact:
        assert p[0] == F32(0.05)
        assert _sel_all(case) != _sel_all(case, ge_threshold=True)
    assert all(len(s[0]) == 20 for s in _sel_all(case))     # the 20 at the edge stay out, the 20 one ulp up are in


def test_tie_cases_discriminate_the_index_order():
    cases = rc.select_cases()
    for name in ("equal_run_at_cut", "same_sigmoid", "toy_one_and_all_equal"):
        assert _sel_all(cases[name]) != _sel_all(cases[name], tie_high_index=True), name
    long = rc.long_cases()["long_spread"]
    assert _sel_all(long) != _sel_all(long, tie_high_index=True)
    xa, xb = rc.same_sigmoid_logits()
    assert xa != xb and ora.map_f32(np.array([xa], F32), 1)[0] == ora.map_f32(np.array([xb], F32), 1)[0]
    # ranking the LOGITS instead of the sigmoids would put the larger logit first
    lg = cases["same_sigmoid"][0][0][0].reshape(-1)
    s, i = rr.select_level(lg)
    assert np.array_equal(i, np.sort(i)) and not np.array_equal(i, i[np.argsort(-lg[i], kind="stable")])


def _post_all(case, flags=0, **kw):
    return [tuple(x.tolist() for x in r) for r in rc.ref_post(case, flags, **kw)]


def test_post_cases_discriminate():
    P = rc.post_cases()
    for name in ("identical_boxes_two_classes", "eighty_classes_5000"):
        assert _post_all(P[name]) != _post_all(P[name], cross_class=True), name
    assert [len(r[1]) for r in _post_all(P["identical_boxes_two_classes"], cross_class=True)] == [1]
    p = rc.iou_04_pair()
    inter, union = F32(20.0), F32(50.0)
    assert inter / union == F32(0.4)
    for flag in (2, 4):     # plain areas, index order: on the clustered boxes (before the cut, so that the whole kept list is compared)
        assert _post_all(P["eighty_classes_5000"], det=0, cap=8192) != _post_all(P["eighty_classes_5000"], flag, det=0, cap=8192), flag
    assert _post_all(P["iou_exactly_thr"]) != _post_all(P["iou_exactly_thr"], 1)     # >= against >: on the pair whose IoU IS the threshold
    assert [len(r[1]) for r in _post_all(P["iou_exactly_thr"])] == [4] and [len(r[1]) for r in _post_all(P["iou_exactly_thr"], 1)] == [2]
    # the cut: `>=` keeps the whole tie group, a strict top-100 would not
    assert [len(r[1]) for r in _post_all(P["cut_tie_group_fits_cap"])] == [115]
    assert [len(r[1]) for r in _post_all(P["cut_tie_group_over_cap"])] == [128]
    assert [len(r[1]) for r in _post_all(P["cut_tie_group_over_cap"], cap=100)] == [100]


# ------------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("depth", [50, 101])
def test_state_dict_and_importer_round_trip(depth):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import import_pth
    from isegmi.weights import maskrcnn_state_dict, retinanet_state_dict
    sd = retinanet_state_dict(3, depth)
    for k in ("backbone.fpn.fpn_inner2.weight", "backbone.fpn.fpn_layer4.bias", "backbone.fpn.top_blocks.p6.weight", "backbone.fpn.top_blocks.p7.bias",
              "rpn.head.cls_tower.0.weight", "rpn.head.bbox_tower.6.bias", "rpn.head.cls_logits.weight", "rpn.head.bbox_pred.bias",
              "backbone.body.layer3.%d.conv2.weight" % (22 if depth == 101 else 5)):
        assert k in sd, k
    assert "backbone.fpn.fpn_inner1.weight" not in sd and "rpn.head.cls_tower.1.weight" not in sd and "rpn.head.conv.weight" not in sd
    assert sd["rpn.head.cls_logits.weight"].shape == (720, 256, 3, 3) and sd["rpn.head.bbox_pred.weight"].shape == (36, 256, 3, 3)
    assert sd["backbone.fpn.top_blocks.p6.weight"].shape == (256, 2048, 3, 3)
    family = "retinanet_r%d_fpn" % depth
    ckpt = {"model": {"module." + k: v for k, v in sd.items()}, "optimizer": {"lr": 0.1}, "iteration": 90000}
    out = import_pth.convert(ckpt, family)
    assert set(out) == set(sd) and all(np.array_equal(out[k], sd[k]) for k in sd)
    with pytest.raises((KeyError, ValueError)):   # a Mask R-CNN checkpoint: other predictor shapes, other keys
        import_pth.convert({"model": maskrcnn_state_dict(3, depth)}, family)
    with pytest.raises(KeyError):
        import_pth.convert(ckpt, "retinanet_r%d_fpn" % (50 if depth == 101 else 101))
    low = retinanet_state_dict(3, depth, cls_bias=-30.0)
    assert np.array_equal(low["rpn.head.cls_logits.weight"], sd["rpn.head.cls_logits.weight"])
    assert np.allclose(low["rpn.head.cls_logits.bias"] - sd["rpn.head.cls_logits.bias"], -25.5, atol=1e-4)


def test_python_refusals_need_no_device():
    from isegmi.retinanet import RetinaNet
    with pytest.raises(ValueError, match="fp16"):
        RetinaNet({}, 256, 352, fp16=True)
    with pytest.raises(ValueError, match="graph"):
        RetinaNet({}, 256, 352, graph=True)


# ------------------------------------------------------------------------------------------------------------------- capacity and threshold edges
def _sel(case, thr=0.05, **kw):
    logits, a, c, top_n = case
    return [[rr.select_level(lg[n], top_n, thr, **kw) for n in range(lg.shape[0])] for lg in logits]


def _same(a, b):
    return all(np.array_equal(x[1], y[1]) and np.array_equal(x[0], y[0]) for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.parametrize("k", rc.TOP_NS)
def test_top_n_cases_hold_more_than_top_n(k):
    case = rc.topn_cases()["topn_%d" % k]
    assert case[3] == k and [lg[0].size for lg in case[0]] == [25200, 4320]
    for lg in case[0]:
        assert rc.candidates(lg[0]) == k + 37 and rc.candidates(lg[1]) == k + 30
        assert len(np.unique(ora.map_f32(lg[0].reshape(-1), 1))) == k + 37 + 1          # all distinct (+ the filler)
    sel, high = _sel(case), _sel(case, tie_high_index=True)
    for l in range(2):
        assert len(sel[l][0][0]) == len(sel[l][1][0]) == k
        assert _same([[sel[l][0]]], [[high[l][0]]]) and not _same([[sel[l][1]]], [[high[l][1]]])   # only the run's winners depend on the tie rule
        s = sel[l][1][0]
        assert s[-1] == ora.map_f32(np.array([0.5], rc.F32), 1)[0] and (s == s[-1]).sum() == k - k // 2     # the cut lies inside the run


def test_top_n_1024_with_exactly_1024_and_1025_candidates():
    case = rc.topn_cases()["topn_1024_exact"]
    assert case[3] == rc.KCAP == 1024
    for lg, row in zip(case[0], _sel(case)):
        assert [rc.candidates(lg[0]), rc.candidates(lg[1])] == [1024, 1025]
        assert len(row[0][0]) == len(row[1][0]) == 1024
        lost = set(np.flatnonzero(lg[1].reshape(-1) > rc.LOW)) - set(row[1][1].tolist())
        assert len(lost) == 1 and lg[1].reshape(-1)[list(lost)[0]] == lg[1].reshape(-1)[lg[1].reshape(-1) > rc.LOW].min()


@pytest.mark.parametrize("n", rc.BORDER_ROWS)
def test_border_cases_reach_both_sides_of_a_slice_border(n):
    S = rc.SLICE
    case = rc.border_cases()["border_distinct_%d" % n]
    row = case[0][0]
    assert row.shape == (2, 1, n, 1) and case[3] == 64
    cand = np.flatnonzero(row[0].reshape(-1) > rc.LOW)
    assert S - 1 in cand or n < S                 # the last index of slice 0 ...
    assert (S in cand) == (n > S)                 # ... and the first of slice 1
    if n > 2 * S:
        assert 2 * S - 1 in cand and 2 * S in cand
    (s0, i0), (s1, i1) = _sel(case)[0]
    assert len(i0) == min(64, cand.size) and set(i0.tolist()) <= set(cand.tolist())
    if n > S:
        assert (i0 < S).any() and (i0 >= S).any()
    assert i1.tolist() == [n - 1]
    # the equal run: the cut falls inside it and its lower indices win
    case = rc.border_cases()["border_tie_%d" % n]
    row = case[0][0]
    run = rc.border_run(n)
    assert run[0] == S - 50 and run[-1] == min(S + 49, n - 1) and (row[0, 0, run, 0] == 0.5).all()
    assert rc.candidates(row[0]) > 64
    (s0, i0), (s1, i1) = _sel(case)[0]
    (h0, j0), _ = _sel(case, tie_high_index=True)[0]
    assert len(i0) == 64 and not np.array_equal(i0, j0)
    won = np.sort(i0[s0 == s0[-1]])
    assert 0 < won.size < run.size and np.array_equal(won, run[:won.size])
    if n >= 2 * S - 1:
        assert won[0] < S and won[-1] > S                     # across the border
        assert not (i0 >= 2 * S - 50).any()                   # the second run, equal in score, loses to the first on the index
    if n == S + 1:
        assert won[-1] == S - 1 and S not in i0               # the first logit of slice 1 ties with the last of slice 0 and loses
    assert i1.tolist() == [n - 1]


def test_geometry_case_counts():
    logits, a, c, top_n = rc.geometry_case()
    assert len(logits) == 5 and a == c == 1 and all(lg.shape[0] == 3 for lg in logits)
    assert [-(-lg[0].size // rc.SLICE) for lg in logits] == [4, 2, 1, 1, 1] and logits[4][0].size == 1
    cnt = np.array([[rc.candidates(lg[n]) for n in range(3)] for lg in logits])
    want = np.array([[lg[0].size if rc.geometry_kind(l, n) < 0 else min(rc.geometry_kind(l, n), lg[0].size) for n in range(3)] for l, lg in enumerate(logits)])
    assert np.array_equal(cnt, want)
    assert {0, 1, top_n, top_n + 1, 25000, 9000, 77} <= set(cnt.reshape(-1).tolist())
    assert all(len(set(row)) > 1 for row in cnt.tolist()) and all(len(set(col)) > 1 for col in cnt.T.tolist())   # a wrong level or image offset shows
    sel = _sel(rc.geometry_case())
    assert np.array_equal([[len(sel[l][n][0]) for n in range(3)] for l in range(5)], np.minimum(cnt, top_n))


SIGMOID_FLOOR = 4.1560284e-39      # what ora.map_f32(x, 1) returns for every logit under about -88.4, -inf included


def test_sigmoid_never_reaches_zero():
    p = ora.map_f32(np.array([-np.inf, -200.0, -104.0, -89.0], rc.F32), 1)
    assert (p == p[0]).all() and p[0] > 0 and abs(float(p[0]) - SIGMOID_FLOOR) < 1e-44


@pytest.mark.parametrize("thr", rc.THRESHOLDS)
def test_threshold_cases(thr):
    """Every threshold: the reference passes some and drops some of the row; the logits the first pre-filter (logit(thr) - 0.25) would have dropped
    although their sigmoid passes are in the row."""
    case = rc.threshold_case(thr)
    row = case[0][0].reshape(-1)
    assert row.size == 4000 and case[3] == 1024
    s, i = rr.select_level(row, 1024, thr)
    numbers = int((~np.isnan(row)).sum())
    assert len(i) == rc.candidates(row, thr) < 1024           # nothing is cut: the list is the whole set that passed
    passed = np.zeros(row.size, bool); passed[i] = True
    if thr <= 0:
        assert len(i) == numbers == len(rc.SPECIALS) - 1      # drops only the NaN
        assert np.isneginf(row[i]).any()
    elif np.float32(thr) < np.float32(SIGMOID_FLOOR):         # the sigmoid's floor is over the threshold: again only the NaN are dropped ...
        assert rc.crossing(thr) is None and len(i) == numbers > 500 and np.isneginf(row[i]).any()
        assert (row[i] <= rc.prefilter_of(thr)).sum() >= 200 + 4     # ... and not the logits at or under logit(thr) - 0.25, the pre-filter as first built
    elif thr >= 1:
        assert len(i) == 0 and numbers > 500
    else:
        assert 0 < len(i) < numbers
        pre = rc.prefilter_of(thr)
        grid = (row >= pre - 1) & (row <= pre + 1)
        assert grid.sum() >= 512 and (row[grid] <= pre).sum() >= 200 and (row[grid] > pre).sum() >= 200
        assert not (passed & (row <= pre)).any()              # the reference passes nothing at or under logit(thr) - 0.25
        x_at, x_up = rc.crossing(thr)
        assert not passed[row == x_at].any() and passed[row == x_up].all() and (row == x_at).sum() == (row == x_up).sum() == 1
    if thr == 0.5:
        assert (row == 0).sum() == 1 and not passed[row == 0].any() and ora.map_f32(np.zeros(1, rc.F32), 1)[0] == 0.5
    if thr == 1.0 - 2.0 ** -24:
        assert len(i) > 0 and (s == 1.0).all()
    assert passed[np.isposinf(row)].all() == (thr < 1) and not passed[np.isnan(row)].any()


def test_crossing_agrees_with_threshold_logits():
    x_at, x_up, _ = rc.threshold_logits()
    assert rc.crossing(0.05) == (x_at, x_up)


def _dec(logits, deltas, anchors, hw, min_size=0.0):
    out = []
    for l in range(len(logits)):
        for n in range(logits[l].shape[0]):
            s, i = rr.select_level(logits[l][n])
            out.append((len(s),) + rr.decode_level(s, i, deltas[l][n], anchors[l], hw[n][1], hw[n][0], min_size=min_size))
    return out


def test_decode_edge_cases():
    d = _dec(*rc.decode_edge_case("tiny_image"))
    assert all(k == len(sc) > 0 and not b.any() for k, b, sc, lb in d)              # every box is (0, 0, 0, 0): 1 wide, kept under min_size 0
    case = rc.decode_edge_case("zero_deltas")
    m, m_up = rc.min_size_edge()
    assert m_up > m > 1
    at, up, none = _dec(*case, min_size=m), _dec(*case, min_size=m_up), _dec(*case, min_size=1e9)
    s, i = rr.select_level(case[0][0][0])
    an = case[2][0][i[0] // rc.C]
    hw = case[3][0]
    clipped = np.clip(an, 0, [hw[1] - 1, hw[0] - 1, hw[1] - 1, hw[0] - 1]).astype(rc.F32)
    assert np.array_equal(at[0][1][0], clipped) and at[0][2][0] == s[0]                  # the decoded box is the clipped anchor, kept at min_size == its side + 1
    assert up[0][2][0] != s[0] and len(up[0][2]) < len(at[0][2]) < at[0][0]              # ... dropped one float above; other boxes were dropped before it
    assert all(len(sc) == 0 and k > 0 for k, b, sc, lb in none)
    case = rc.decode_edge_case("special_deltas")
    d = _dec(*case)
    q = 0
    for l in range(len(case[0])):
        for n in range(2):
            s, i = rr.select_level(case[0][l][n])
            nan_centre = np.isin(i // rc.C, (1, 7))                                         # dx / dy NaN: a NaN box, which fails `>= min_size`
            k, b, sc, lb = d[q]; q += 1
            assert k - len(sc) == nan_centre.sum() >= 2 and np.array_equal(sc, s[~nan_centre])
            assert np.isfinite(b).all()                                                      # +-inf clip to the border; a NaN dw takes the clamp's value
            assert set(range(rc.A)) <= set((i // rc.C).tolist())                             # all nine special anchors are among the selected
    assert all(k == len(sc) for k, b, sc, lb in _dec(*rc.decode_edge_case("zero_deltas")))


def _labels_clipped(case):
    nc = case.get("ncls", 81) - 1
    return dict(case, l=[np.clip(x, 1, nc) for x in case["l"]])


def test_full_cases_reach_the_capacity():
    F = rc.full_cases()
    for name in ("full_one_class", "full_100_then_8092", "full_255_classes"):
        c = F[name]
        B, S, Lb, cnt = rc.pack_post(c)
        assert B.shape == (1, 8, 1024, 4) and (cnt == 1024).all()                         # every slot valid
        assert ((c["l"][0] >= 1) & (c["l"][0] < c.get("ncls", 81))).all()
    r = rc.class_reach(F["full_one_class"], 17)
    assert (r["s"], r["e"], r["words"]) == (0, 8192, 128) and r["far"] and r["upper"] and r["last"], r
    r = rc.class_reach(F["full_100_then_8092"], 2)
    assert (r["s"], r["e"], r["words"]) == (100, 8192, 127) and r["s"] % 64 != 0 and r["far"] and r["upper"] and r["last"], r
    c = F["full_255_classes"]
    assert c["ncls"] == 256 and c["l"][0].max() == 255
    r = rc.class_reach(c, 255)
    assert (r["s"], r["e"], r["words"]) == (4092, 8192, 65) and r["s"] % 64 != 0 and r["upper"] and r["last"], r    # rel crosses 64 with w0 = 63
    assert rc.class_reach(c, 254)["s"] == 4055 and rc.class_reach(c, 1)["last"]
    for name in ("full_one_class", "full_100_then_8092", "full_255_classes"):
        uncut, cut = rc.full_ref(name, 0, 8192)[0], rc.full_ref(name, 100, 128)[0]
        assert 1000 < len(uncut[1]) < 8192 and 100 <= len(cut[1]) <= 128
    b = F["batch_8192_0_1"]
    assert [len(s) for s in b["s"]] == [8192, 0, 1] and rc.pack_post(b)[3].sum(1).tolist() == [8192, 0, 1]
    assert [len(r[1]) for r in rc.full_ref("batch_8192_0_1", 100, 128)][1:] == [0, 1]


def test_edge_post_cases_discriminate():
    P = rc.edge_post_cases()
    assert P["ncls_2"]["ncls"] == 2 and 0 < len(_post_all(P["ncls_2"])[0][1]) < 60
    for ncls in (2, 81):
        c = P["labels_out_of_range_ncls_%d" % ncls]
        got = _post_all(c)[0]
        assert got[2] == [1] * 6 and len(set(c["l"][0][0::2].tolist()) & set(range(1, ncls))) == 0
        assert max(got[1]) < 0.7                                              # only the worse twin of each pair
        clipped = _post_all(_labels_clipped(c))[0]                            # counted into a class, the better twins would appear and suppress theirs
        assert clipped != got and max(clipped[1]) > 0.8 and (ncls == 81 or len(clipped[1]) == 6)
        B, S, Lb, cnt = rc.pack_post(c)
        past = Lb[0][np.arange(8)[None, :] >= cnt[0][:, None]]
        assert ((past >= 1) & (past < ncls)).any() and ((past < 1) | (past >= ncls)).any()
    K = rc.CUT_K
    for name, dets, counts in (("cut_k40", (1, K - 1, K, K + 1), (1, K, K, K)), ("cut_k40_zeros", (1, 32, K - 1, K, K + 1), (1, 34, K, K, K))):
        assert [len(_post_all(P[name], det=d, cap=64)[0][1]) for d in dets] == list(counts), name
        assert len(_post_all(P[name], det=0, cap=64)[0][1]) == K
    z = P["cut_k40_zeros"]["s"][0]
    assert (np.signbit(z) & (z == 0)).sum() == 2 and (~np.signbit(z) & (z == 0)).sum() == 2 and (z < 0).sum() == 6
