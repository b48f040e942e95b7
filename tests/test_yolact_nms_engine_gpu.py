"""The Yolact engine in nms_mode 1 (cross-class fast NMS) and 2 (traditional NMS): detections, masks and integer boxes bit for bit against
YolactRef's head outputs run through the restated tails (tests/yolact_nms_ref.py); lazy coefficients, the graph form, YOLACT++ re-scoring, the
record path with a forced capacity overflow, the command line and the engine-level refusals.

Random weights: the class scores sit near 1/81 and the decoded boxes overlap little, so the configs here lower nms_conf_thresh to 0.012 (< 1/81)
and nms_thresh to 0.15 -- chosen on the CPU so that many classes hold several candidates and every image's result differs from the default rule's."""
import dataclasses
import json
import os

import numpy as np
import pytest

import yolact_nms_ref as R
from oracle import ora
from oracle.yolact_ref import YolactRef

pytestmark = pytest.mark.gpu
CONF, THR, SIZE = 0.012, 0.15, 200


def _cfg(mode, base=None, **kw):
    from isegmi.yolact import YolactConfig
    base = base or YolactConfig()
    return dataclasses.replace(base, nms_conf_thresh=CONF, nms_thresh=THR, use_fast_nms=mode != 2, use_cross_class_nms=mode == 1, **kw)


@pytest.fixture(scope="module")
def sd():
    from isegmi.weights import yolact_state_dict
    return yolact_state_dict(1234)


@pytest.fixture(scope="module")
def batch():
    from isegmi.yolact import fast_base_transform
    return fast_base_transform(np.random.default_rng(0).uniform(0, 255, (3, SIZE, SIZE, 3)).astype(np.float32))


def _tails(ref, n_images, max_size=550, cap=1024):
    """the reference head outputs through the default rule and the two restated ones, per image: {mode: [(det, total, overflow)]}"""
    f = ref.feats
    out = {0: [], 1: [], 2: []}
    for n in range(n_images):
        prob = ora.softmax(f["conf"][n]); boxes = ora.yolact_decode(f["loc"][n], f["priors"])
        out[0].append((ora.yolact_detect(prob, boxes, f["mask"][n], CONF, THR), None, 0))
        for mode in (1, 2):
            d, t, o = R.run_ref(mode, prob, boxes, f["mask"][n], CONF, THR, 200, 100, max_size, cap)
            d["proto"] = f["proto"][n]
            out[mode].append((d, t, o))
        cnt = (prob[:, 1:] > np.float32(CONF)).sum(0)
        assert (cnt >= 5).sum() >= 5, "few classes hold several candidates"
    return out


@pytest.fixture(scope="module")
def ref(sd, batch):
    r = YolactRef(sd)
    r.forward(batch)
    return r


@pytest.fixture(scope="module")
def tails(ref):
    t = _tails(ref, 3)
    for mode in (1, 2):   # the modes are told apart: some image's result differs from the default rule's, and nothing overflows the default cap
        assert any(not R.same(t[0][n][0], t[mode][n][0]) for n in range(3))
        assert not any(t[mode][n][2] for n in range(3))
    return t


def _compare(out, want, size=SIZE):
    from isegmi.yolact import postprocess
    for i, (d, total, _) in enumerate(want):
        det = out[i]["detection"]
        assert det is not None and len(det["score"]) == len(d["score"]) > 0
        for a, b in (("prior", "prior"), ("class", "cls"), ("score", "score"), ("box", "box"), ("mask", "mask")):
            assert np.array_equal(det[a], d[b]), (i, a)
        assert out[i]["nms_total"] == total
        cls, sc, boxes, masks = postprocess(out, size, size, batch_idx=i)
        rc, rs, rb, rm = YolactRef.postprocess(d, size, size)
        if isinstance(sc, list):
            sc = sc[0]
        assert np.array_equal(cls, rc) and np.array_equal(sc, rs) and np.array_equal(boxes, rb) and np.array_equal(masks, rm), i


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
def test_engine_matches_restated_tail(ffi, sd, batch, tails, mode, lazy):
    """batch 1 and 3 on one engine; lazy_coeffs works in both modes (the final top-k's indices resolve through the mode's own index rows)"""
    from isegmi.yolact import Yolact
    net = Yolact(sd, _cfg(mode), max_batch=3, input_size=SIZE)
    net.set_param("lazy_coeffs", float(lazy))
    for b in (1, 3):
        _compare(net(batch[:b]), tails[mode][:b])
    if lazy:
        assert net.fetch("ws.coeff_sel", 3).shape == (3, 100, 32)
    net.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_engine_one_stream_and_back_to_back_steps(ffi, sd, batch, tails, mode):
    """multi_stream 0 (everything on one stream), then the default multi-stream form with two forwards enqueued before the first sync (the
    second step's backbone runs under the first one's Detect tail)"""
    from isegmi.yolact import Yolact
    net = Yolact(sd, _cfg(mode), max_batch=3, input_size=SIZE)
    net.set_param("multi_stream", 0.0)
    _compare(net(batch), tails[mode])
    net.set_param("multi_stream", 1.0)
    n = net.upload(batch)
    net.forward_device(n)
    net.forward_device(n)
    _compare(net(batch), tails[mode])
    net.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_engine_fp16_storage(ffi, sd, batch, mode):
    """fp16 storage keeps the heads and Detect in fp32: the engine's own head outputs (`headcat`) through the restated tail give its detections"""
    from isegmi.yolact import Yolact
    net = Yolact(sd, _cfg(mode), max_batch=2, input_size=SIZE, fp16=True)
    out = net(batch[:2])
    hc = net.fetch("headcat", 2)
    A, P = 3, net.priors.shape[0]
    loc = hc[..., :A * 4].reshape(2, P, 4); conf = hc[..., A * 4:A * 85].reshape(2, P, 81); mask = hc[..., A * 85:A * 117].reshape(2, P, 32)
    for n in range(2):
        d, total, over = R.run_ref(mode, ora.softmax(conf[n]), ora.yolact_decode(loc[n], net.priors), mask[n], CONF, THR, 200, 100, 550, 1024)
        det = out[n]["detection"]
        assert len(d["score"]) > 0 and not over and out[n]["nms_total"] == total
        for a, b in (("prior", "prior"), ("class", "cls"), ("score", "score"), ("box", "box")):   # (the coefficients pass through tanh on the device)
            assert np.array_equal(det[a], d[b]), (n, a)
    net.close()


def test_mode_selected_with_set_param_is_checked_too(ffi, sd, batch):
    """an engine built with the default config and switched with set_param reads det.nms_overflow as one built from the config does"""
    from isegmi.yolact import NmsCapOverflow, Yolact, YolactConfig
    net = Yolact(sd, dataclasses.replace(YolactConfig(), nms_conf_thresh=CONF, nms_thresh=THR), max_batch=1, input_size=SIZE)
    assert net.nms_mode == 0 and "nms_total" not in net(batch[:1])[0]
    net.set_param("max_size", 550.0); net.set_param("nms_mode", 2.0); net.set_param("nms_trad_cap", 64.0)
    assert net.nms_mode == 2 and net.nms_trad_cap == 64
    with pytest.raises(NmsCapOverflow, match="nms_trad_cap = 64"):
        net(batch[:1])
    net.set_param("nms_trad_cap", 1024.0)
    assert net(batch[:1])[0]["nms_total"] > 0
    net.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_engine_graph_form(ffi, sd, batch, tails, mode):
    from isegmi.yolact import Yolact
    net = Yolact(sd, _cfg(mode), max_batch=2, input_size=SIZE)
    net.set_param("graph", 1.0)
    for _ in range(3):   # capture, then replays
        _compare(net(batch[:2]), tails[mode][:2])
    net.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_engine_yolact_plus_rescoring(ffi, mode):
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, YolactConfig, fast_base_transform, postprocess
    base = YolactConfig.plus_resnet50()
    size = 256   # the smallest input whose prototypes survive the mask-IoU net
    sdp = yolact_state_dict(77, depth=50, num_priors=9, dcn_layers=base.dcn_layers, dcn_interval=base.dcn_interval, maskiou=True)
    x = fast_base_transform(np.random.default_rng(91).uniform(0, 255, (1, size, size, 3)).astype(np.float32))
    ref = YolactRef(sdp, max_size=550, depth=50, scales_per_level=3, square=False)
    ref.forward(x)
    f = ref.feats
    d, total, over = R.run_ref(mode, ora.softmax(f["conf"][0]), ora.yolact_decode(f["loc"][0], f["priors"]), f["mask"][0], CONF, THR, 200, 100, 550, 1024)
    d["proto"] = f["proto"][0]
    assert len(d["score"]) > 0 and not over
    net = Yolact(sdp, _cfg(mode, base), max_batch=1, input_size=size)
    out = net(x)
    _compare(out, [(d, total, over)], size)
    sc = postprocess(out, size, size)[1]
    assert isinstance(sc, list) and np.array_equal(sc[1], ref.mask_scores(d, 0.0))
    net.close()


def test_overflow_raises_and_names_the_parameter(ffi, sd, batch, ref):
    from isegmi.yolact import NmsCapOverflow, Yolact
    want = [o for _, _, o in _tails(ref, 3, cap=64)[2]]
    assert any(want)
    net = Yolact(sd, _cfg(2, nms_trad_cap=64), max_batch=3, input_size=SIZE)
    n = net.upload(batch)
    net.forward_device(n)
    net.sync()
    assert net.fetch("det.nms_overflow", 3).tolist() == want
    with pytest.raises(NmsCapOverflow, match="nms_trad_cap"):
        net(batch)
    net.close()


def test_record_loop_recovers_from_a_forced_overflow(ffi, sd):
    """evaluate() with nms_trad_cap = 64: the step's records carry the flag, the loop doubles the capacity and redoes the step until the flag is
    clear; the result is the default capacity's"""
    from isegmi.yolact import Yolact, evaluate
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (SIZE, SIZE, 3)).astype(np.uint8) for _ in range(2)]
    net = Yolact(sd, _cfg(2), max_batch=2, input_size=SIZE)
    want = evaluate(net, images, batch_size=2, top_k=20)
    net.close()
    net = Yolact(sd, _cfg(2, nms_trad_cap=64), max_batch=2, input_size=SIZE)
    got = evaluate(net, images, batch_size=2, top_k=20)
    assert net.nms_trad_cap > 64
    net.close()
    assert len(want) == 40 and json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)


def test_cli_eval_traditional(ffi, tmp_path):
    """eval --fast_nms False --images ... writes its json (random weights at the default thresholds: the run and the file, not the content)"""
    from PIL import Image
    from isegmi.cli import main
    src = tmp_path / "in"; dst = tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(1)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (64, 80, 3)).astype(np.uint8)).save(str(src / ("%d.png" % i)))
    js = tmp_path / "dets.json"
    main(["eval", "--fast_nms", "False", "--images", "%s:%s" % (src, dst), "--output_coco_json", str(js), "--batch_size", "2"])
    assert os.path.exists(js) and isinstance(json.load(open(js)), list)


@pytest.mark.parametrize("params,name", [(dict(nms_mode=3), "nms_mode"), (dict(nms_mode=2, nms_trad_cap=100), "nms_trad_cap"),
                                         (dict(nms_mode=2, nms_trad_cap=4096), "nms_trad_cap"),
                                         (dict(nms_mode=1, nms_second_threshold=1), "nms_second_threshold"),
                                         (dict(nms_mode=2, nms_second_threshold=1), "nms_second_threshold")])
def test_engine_refusals_name_the_parameter(ffi, sd, batch, params, name):
    from isegmi.yolact import Yolact
    net = Yolact(sd, max_batch=1, input_size=SIZE)
    for k, v in params.items():
        net.set_param(k, float(v))
    n = net.upload(batch[:1])
    with pytest.raises(Exception, match=name):
        net.forward_device(n)
    for k in params:   # and the engine is usable afterwards
        net.set_param(k, {"nms_trad_cap": 1024.0}.get(k, 0.0))
    net.forward_device(n)
    net.sync()
    assert int(net.fetch("det.count", 1)[0]) > 0
    net.close()
