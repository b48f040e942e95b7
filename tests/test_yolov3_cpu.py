"""YOLOv3 on the CPU: the hand-derived pins of the contract against the oracle, the host side (config, .cfg, .weights, letterbox, command line, COCO
json), and -- with tests/yolov3_ref.py alone -- that every crafted input of tests/yolov3_cases.py reaches the limit or discriminates the rule it is named for."""
import dataclasses
import json
import os

import numpy as np
import pytest

import retinanet_ref as rr
import yolov3_cases as yc
import yolov3_ref as yr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(c, **forks):
    kw = dict(c)
    heads = kw.pop("heads")
    kw.update(forks)
    return yr.select_decode(heads, **kw)


def _same(a, b):
    return all(len(x[1]) == len(y[1]) and np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
               for ra, rb in zip(a, b) for x, y in zip(ra, rb))


# ---------------------------------------------------------------------------------------------------------------- pins
def test_pins_against_the_oracle():
    assert yr.exp([0.0])[0] == F32(1.0) and yr.sigmoid([0.0])[0] == F32(0.5)
    assert yr.sigmoid([yc.ON])[0] == F32(1.0) and yr.sigmoid([88.0])[0] == F32(1.0)
    floor = yr.sigmoid([-np.inf])[0]
    assert 0 < floor < np.finfo(F32).tiny and abs(float(floor) - 4.156e-39) < 1e-41
    assert yr.exp([np.inf])[0] > F32(2.4e38) and np.isfinite(yr.exp([np.inf])[0])   # dm_exp saturates at 2.406e38
    # all-zero t at cell (x 1, y 0), stride 32, anchor (116, 90): centre (48, 16), box (-10, -29, 106, 61) before the clip
    cx, cy = (yr.sigmoid([0.0])[0] + F32(1)) * F32(32), (yr.sigmoid([0.0])[0] + F32(0)) * F32(32)
    hw, hh = yr.exp([0.0])[0] * F32(116) * F32(0.5), yr.exp([0.0])[0] * F32(90) * F32(0.5)
    assert (cx, cy) == (48, 16) and (cx - hw, cy - hh, cx + hw, cy + hh) == (-10, -29, 106, 61)
    h = yc.empty_head(1, 1, 2, 3, 1)
    h[0, 0, 1, 0, 4:] = yc.ON
    dec, total = _run(yc.case([h], canvas_w=416, canvas_h=416))
    b, s, lab = dec[0][0]
    assert total.tolist() == [[1]] and s.tolist() == [1.0] and lab.tolist() == [1] and b.tolist() == [[0, 0, 106, 61]]


def test_objectness_is_an_exact_prefilter():
    """obj * p <= obj in rounded fp32 for every class sigmoid p: s > thr implies obj > thr."""
    rng = np.random.default_rng(5)
    logits = np.concatenate([rng.normal(0, 8, 20000), rng.uniform(-100, 100, 20000), [-np.inf, np.inf, 0, 88, -88, 16.7, 17.0]]).astype(F32)
    p = yr.sigmoid(logits)
    assert (p <= 1).all() and (p > 0).all()
    bits = rng.integers(1, 0x3f800000, 40007, dtype=np.uint32)   # every positive float up to 1.0, subnormals included
    obj = np.concatenate([bits.view(F32), yr.sigmoid(rng.normal(0, 6, 20000).astype(F32))])
    for o in (obj[:: 7], obj[3:: 11]):
        q = p[rng.integers(0, p.size, o.size)]
        assert ((o * q).astype(F32) <= o).all()
    assert (F32(1.0) * p == p).all()


# ---------------------------------------------------------------------------------------------------------------- the crafted inputs
def test_cases_reach_their_limits():
    for top_n in yc.TOP_NS:
        for kind in ("distinct", "tie"):
            c = yc.count_cases()["count_%s_top%d" % (kind, top_n)]
            dec, total = _run(c)
            plan = np.asarray(yc.count_plan(top_n)).T
            assert np.array_equal(total, plan)
            kept = np.asarray([[len(dec[l][n][1]) for l in range(3)] for n in range(2)])
            assert np.array_equal(kept, np.minimum(plan, top_n))
            s = dec[2][0][1]
            assert (len(np.unique(s)) == len(s)) == (kind == "distinct" or top_n == 1)
    for C in (1, 80):
        rs = yc.slice_records(C)
        assert rs * (5 + C) <= yc.SLICE_FLOATS < (rs + 1) * (5 + C)
        for name, nrec in zip(yc.BORDER_ROWS, (rs - 1, rs, rs + 1, 2 * rs + 1)):
            c = yc.slice_cases()["slice_C%d_%s" % (C, name)]
            assert c["heads"][0].shape[2] == nrec
            cand = np.flatnonzero(yr.scores(c["heads"][0][1], 1) > F32(0.5)) // C
            assert {0, nrec - 1} <= set(cand) and all(r in cand for r in (rs - 1, rs, 2 * rs - 1, 2 * rs) if r < nrec)
    dec, total = _run(yc.slice_cases()["slice_C80_two_plus1"])
    assert total.tolist() == [[7], [7]] and len(dec[0][0][1]) == 3 and len(set(dec[0][0][1].tolist())) == 1   # the cut runs through an equal-score run
    t = yc.threshold_cases()
    assert [int(_run(t["thr_%s_product" % k])[1].sum()) for k in ("pred", "at", "succ")] == [1, 0, 0]
    assert int(_run(t["thr_objectness_at_threshold"])[1].sum()) == 0 and int(_run(t["thr_objectness_above_threshold"])[1].sum()) == 1
    assert _run(t["thr_zero"])[1].tolist() == [[34], [36]]          # every pair but the two whose product underflows to 0
    assert _run(t["thr_one"])[1].tolist() == [[0], [0]]
    assert _run(t["thr_below_sigmoid_floor"])[1].tolist()[1] in ([35], [36])
    assert F32(t["thr_below_sigmoid_floor"]["thr"]) == np.nextafter(yr.sigmoid([-np.inf])[0], F32(0)) > 0
    e = yc.edge_cases()
    dec, total = _run(e["decode_inf_nan"])
    b = dec[0][0][0]
    assert total.tolist() == [[5]] and len(b) == 3 and (b[:, 2] - b[:, 0]).tolist().count(64.0) == 1 and (b[:, 2] - b[:, 0]).tolist().count(0.0) == 1
    assert [16.0, 30.0] in np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).tolist()
    assert [len(_run(e[k])[0][0][0][1]) for k in ("min_wh_equal_side", "min_wh_one_float_above", "every_box_dropped")] == [2, 1, 0]
    g = yc.geometry_cases()
    assert len(g) == 24 and {c["heads"][0].shape[0] for c in g.values()} == {1, 3} and {len(c["heads"]) for c in g.values()} == {1, 3}
    assert {c["heads"][0].shape[1:3] for c in g.values() if len(c["heads"]) == 1} == set(yc.GRIDS)


def test_wrong_rules_give_other_answers():
    t, e = yc.threshold_cases(), yc.edge_cases()
    assert int(_run(t["thr_at_product"], ge_threshold=True)[1].sum()) == 1                       # >= instead of >
    c = yc.count_cases()["count_tie_top64"]
    assert not _same(_run(c)[0], _run(c, tie_high_index=True)[0])                                # the higher index of equal scores
    c = e["best_class_equal_sigmoids"]
    right, wrong = _run(c)[0][0][0], _run(c, best_by_logit=True)[0][0][0]
    assert 3 in right[2] and 6 not in right[2] and 6 in wrong[2] and 3 not in wrong[2]           # labels are class + 1
    assert len(_run(e["multi_label_same_input"])[0][0][0][1]) > len(right[1])
    c = yc.geometry_cases()["geom_nl1_C2_N1_g0"]
    assert c["heads"][0].shape[1] != c["heads"][0].shape[2] and not _same(_run(c)[0], _run(c, swap_xy=True)[0])   # x / y swapped
    a, b = np.arange(32, dtype=F32).reshape(1, 1, 1, 32), -np.arange(128, dtype=F32).reshape(1, 2, 2, 32)
    out = yr.concat_up2x(a, b)
    assert out.shape == (1, 2, 2, 64) and np.array_equal(out[0, 1, 0, :32], a[0, 0, 0]) and np.array_equal(out[0, 1, 0, 32:], b[0, 1, 0])
    assert not np.array_equal(out, yr.concat_up2x(a, b, swap_concat=True))


def test_chain_case_has_work_for_nms():
    c = dict(yc.chain_case())
    heads = c.pop("heads")
    dec, total, dets = yr.tail(heads, **c)
    for n in range(3):
        cand = sum(len(d[n][1]) for d in dec)
        assert all(len(d[n][1]) > 0 for d in dec) and 0 < len(dets[n][1]) < cand


@pytest.mark.parametrize("canvas", yc.ENGINE_CANVASES)
def test_engine_seed_gives_the_tail_work(canvas):
    """In the reference alone: every image keeps a detection, every level contributes a candidate, NMS removes a box."""
    ref, dets = yc.engine_reference(*canvas)
    dec = ref.feats["dec"]
    assert [h.shape[1:3] for h in ref.feats["heads"]] == [(canvas[0] // s, canvas[1] // s) for s in (32, 16, 8)]
    for n in range(2):
        assert len(dets[n]["score"]) >= 1 and all(len(d[n][1]) >= 1 for d in dec)
        allb = [np.concatenate([d[n][k] for d in dec]) for k in range(3)]
        survivors = rr.postprocess(*allb, 0.4, 0, 4096, 2, 81, return_total=True)[3]
        assert survivors < len(allb[1])


# ---------------------------------------------------------------------------------------------------------------- config, .cfg, refusals
def test_config_and_cfg_refusals_name_their_key():
    from isegmi.config import parse_darknet_cfg, yolov3_cfg_text
    from isegmi.yolov3 import YoloV3, YoloV3Config
    cfg = YoloV3Config()
    assert cfg.level_anchors().tolist() == yr.ANCHORS.tolist() and cfg.det_cap == 100 and cfg.conf_thresh == 0.5 and cfg.nms_thresh == 0.4
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.classes = 3
    for key, kw in (("height", dict(height=400)), ("width", dict(width=1056)), ("classes", dict(classes=0)), ("classes", dict(classes=256)),
                    ("pre_nms_top_n", dict(pre_nms_top_n=1025)), ("pre_nms_top_n", dict(pre_nms_top_n=0)), ("masks", dict(masks=((6, 7), (3, 4), (0, 1)))),
                    ("conf_thresh", dict(conf_thresh=-0.1)), ("min_wh", dict(min_wh=float("nan")))):
        with pytest.raises(ValueError, match=key):
            dataclasses.replace(cfg, **kw).validate()
    with pytest.raises(ValueError, match="fp16"):
        YoloV3({}, fp16=True)
    with pytest.raises(ValueError, match="graph"):
        YoloV3({}, graph=True)
    with pytest.raises(ValueError, match="pre_nms_top_n"):
        YoloV3({}, cfg=dataclasses.replace(cfg, pre_nms_top_n=1025))
    text = open(os.path.join(ROOT, "configs", "yolov3.cfg")).read()
    assert parse_darknet_cfg(text) == cfg and parse_darknet_cfg(text, conf_thresh=0.1).conf_thresh == 0.1
    assert text.count("[convolutional]") == 75 and text.count("[yolo]") == 3 and text.count("[shortcut]") == 23
    assert parse_darknet_cfg(yolov3_cfg_text(dataclasses.replace(cfg, classes=20, height=608, width=320))).classes == 20
    for match, bad in ((r"\[maxpool\]", text.replace("[upsample]\nstride=2", "[maxpool]\nsize=2\nstride=1", 1)),
                       (r"section 81 \[convolutional\].*254", text.replace("filters=255", "filters=254", 1)),
                       (r"mask=6,7", text.replace("mask=6,7,8", "mask=6,7")),
                       (r"section 86 \[route\]", text.replace("layers=-1, 61", "layers=-1, 60")),
                       (r"three", text[: text.rindex("[route]")]),
                       (r"\[net\]", text[text.index("[convolutional]"):])):
        with pytest.raises(ValueError, match=match):
            parse_darknet_cfg(bad)


# ---------------------------------------------------------------------------------------------------------------- .weights
def test_darknet_weights_round_trip_and_length_checks(tmp_path):
    from isegmi.weights import load_darknet_weights, save_darknet_weights, yolov3_layers
    from isegmi.yolov3 import YoloV3Config, yolov3_folded
    sd = yc.engine_weights()
    layers = yolov3_layers(80)
    assert len(layers) == 75 and sum(1 for l in layers if l[1] is None) == 3 and layers[58][0] == "head.0.conv6" and layers[59][0] == "head.1.route"
    assert [l[3] for l in layers if l[0] in ("head.1.conv0", "head.2.conv0")] == [768, 384]
    path = str(tmp_path / "yolov3.weights")
    save_darknet_weights(sd, path)
    nfloat = sum(co * ci * k * k + (4 * co if bn else co) for _, bn, co, ci, k in layers)
    assert os.path.getsize(path) == 20 + 4 * nfloat
    back = load_darknet_weights(path, YoloV3Config())
    assert sorted(back) == sorted(sd) and all(np.array_equal(back[k], sd[k]) and back[k].dtype == np.float32 for k in sd)
    with open(path, "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match="too long.*head.2.conv6"):
        load_darknet_weights(path)
    os.truncate(path, 20 + 4 * (nfloat - 10))
    with pytest.raises(ValueError, match=r"too short.*head\.2\.conv6 \(weight\)"):
        load_darknet_weights(path)
    os.truncate(path, 20 + 4 * 40)
    with pytest.raises(ValueError, match=r"too short.*backbone\._preconv\.0 \(BN\.weight\)"):
        load_darknet_weights(path)
    # bn_eps is the switch between the PyTorch ports (1e-5) and darknet's normaliser (1e-6)
    small = {k: v for k, v in sd.items()}
    a = yolov3_folded(small, YoloV3Config(bn_eps=1e-5))["head.0.conv0"]
    b = yolov3_folded(small, YoloV3Config(bn_eps=1e-6))["head.0.conv0"]
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    assert a[0].shape == (512, 1, 1, 1024) and yolov3_folded(small)["head.2.conv6"][1] is None


# ---------------------------------------------------------------------------------------------------------------- letterbox
@pytest.mark.parametrize("hw", [(1, 1), (31, 64), (64, 31)])
@pytest.mark.parametrize("canvas", [(64, 96), (96, 64), (416, 416)])
def test_letterbox_and_back_mapping(hw, canvas):
    from isegmi.transforms import letterbox_geometry, yolo_letterbox, yolo_unletterbox
    h, w = hw
    S_h, S_w = canvas
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    x, (gain, px, py) = yolo_letterbox(img, S_h, S_w)
    g2, nh, nw, px2, py2 = letterbox_geometry(h, w, S_h, S_w)
    assert (gain, px, py) == (g2, px2, py2) and gain == min(S_h / h, S_w / w) and (nh, nw) == (round(h * gain), round(w * gain))
    assert x.shape == (S_h, S_w, 3) and x.dtype == np.float32 and 0 <= x.min() and x.max() <= 1
    assert nh == S_h or nw == S_w                                                    # one side fills the canvas
    assert 0 <= (S_w - nw) - 2 * px <= 1 and 0 <= (S_h - nh) - 2 * py <= 1           # centred: the slack splits evenly, the odd pixel goes right / bottom
    pad = np.ones((S_h, S_w), bool)
    pad[py:py + nh, px:px + nw] = False
    assert (x[pad] == F32(0.5)).all()
    if hw == (1, 1):
        assert (x[~pad].reshape(-1, 3) == (img[0, 0, ::-1].astype(F32) / F32(255))).all()               # RGB, x / 255
    # a box maps back onto itself: forward in fp32, back through yolo_unletterbox; the error is a few roundings of a canvas coordinate, divided by gain
    box = np.asarray([[0, 0, w, h], [w * 0.25, h * 0.5, w * 0.75, h], [0.3, 0.1, 0.9, 0.7]], F32)
    fwd = box * F32(gain) + np.asarray([px, py, px, py], F32)
    back = yolo_unletterbox(fwd, (gain, px, py), h, w)
    tol = 4 * np.spacing(F32(max(S_h, S_w))) / gain
    assert back.dtype == np.float32 and np.abs(back - np.clip(box, 0, [w, h, w, h])).max() <= tol
    out = yolo_unletterbox(np.asarray([[-5, -5, S_w + 5, S_h + 5]], F32), (gain, px, py), h, w)
    assert out.tolist() == [[0, 0, w, h]]                                            # clipped to the original image


# ---------------------------------------------------------------------------------------------------------------- command line, json
def test_yolo_detect_arguments_and_config():
    from isegmi.cli import build_parser, yolo_config
    cfgp = os.path.join(ROOT, "configs", "yolov3.cfg")
    a = build_parser().parse_args(["yolo_detect", "--cfg", cfgp, "--weights", "random", "--images", "DIR", "--img-size", "416", "--conf-thres", "0.25",
                                   "--nms-thres", "0.45", "--output", "dets.json", "--gt", "instances.json"])
    assert (a.cmd, a.weights, a.images, a.img_size, a.output, a.gt) == ("yolo_detect", "random", "DIR", [416], "dets.json", "instances.json")
    y = yolo_config(a)
    assert (y.height, y.width, y.conf_thresh, y.nms_thresh, y.multi_label, y.bn_eps) == (416, 416, 0.25, 0.45, True, 1e-5)
    a = build_parser().parse_args(["yolo_detect", "--cfg", cfgp, "--images", "D", "--img-size", "64", "96", "--best-class", "--bn-eps", "1e-6"])
    y = yolo_config(a)
    assert (y.height, y.width, y.conf_thresh, y.multi_label, y.bn_eps, a.output, a.batch_size) == (64, 96, 0.5, False, 1e-6, "dets.json", 8)
    with pytest.raises(ValueError, match="height"):
        yolo_config(build_parser().parse_args(["yolo_detect", "--cfg", cfgp, "--images", "D", "--img-size", "100"]))
    with pytest.raises(SystemExit):
        build_parser().parse_args(["yolo_detect", "--cfg", cfgp])


def test_yolo_detect_refuses_more_than_one_rank(monkeypatch):
    from isegmi.cli import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="world > 1"):
        main(["yolo_detect", "--cfg", os.path.join(ROOT, "configs", "yolov3.cfg"), "--images", "D"])


def test_coco_json_has_plain_widths():
    from isegmi.coco import COCO_CATEGORY_IDS, label_categories, yolo_results
    r = yolo_results(7, [[1.5, 2.0, 11.5, 22.0], [0, 0, 3, 4]], [0.9, 0.25], [1, 80])
    assert r[0] == {"image_id": 7, "category_id": COCO_CATEGORY_IDS[0], "bbox": [1.5, 2.0, 10.0, 20.0], "score": pytest.approx(0.9)}
    assert r[1]["category_id"] == COCO_CATEGORY_IDS[79] == 90 and r[1]["bbox"] == [0.0, 0.0, 3.0, 4.0]
    assert yolo_results(0, [[0, 0, 1, 1]], [1.0], [3], label_categories(21))[0]["category_id"] == 3
    json.dumps(r)
