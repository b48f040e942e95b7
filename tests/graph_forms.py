"""The graph manifest (TEST INFRASTRUCTURE ONLY; tools/graph_manifest.py records it, tests/test_graph_manifest_gpu.py compares against it): one form per
branch of the R-CNN and RetinaNet graph code (csrc/maskrcnn.cpp, csrc/retinanet.cpp), each run on a small seeded synthetic model, and what a form leaves
behind -- the stage marks, the op and conv statistics, the conv launch order per forward, the buffers and a hash of the detections.  The manifest pins the
graph code's launches, buffers and results while that code is restructured: every field is compared with exact equality."""
import ctypes as C
import dataclasses
import functools
import hashlib
import json

import numpy as np

# ---- images: canvas name -> list of images (BGR 0..255 float, already resized) and the divisibility they are padded to
@functools.lru_cache(maxsize=None)
def _tiny():
    return [np.random.default_rng(20261018).uniform(0, 255, (100, 130, 3)).astype(np.float32),
            np.random.default_rng(20261019).uniform(0, 255, (120, 150, 3)).astype(np.float32)]


def images(canvas):
    """-> (list of images, divisibility)"""
    if canvas == "tiny":        # 128 x 160
        return _tiny(), 32
    if canvas == "tiny_b":      # 128 x 128: the tiny images cropped
        return [_tiny()[0][:100, :110], _tiny()[1][:120, :100]], 32
    if canvas == "small":       # 256 x 352
        import maskrcnn_gn_common as gc
        return gc.small_images(), 32
    if canvas == "kp":          # 128 x 160, the keypoint suite's images
        from test_keypointrcnn_gpu import _batch
        x, hw = _batch()
        return (x, hw), 32
    if canvas == "c4":          # 208 x 272
        return [np.random.default_rng(5).uniform(0, 255, (200, 260, 3)).astype(np.float32)], 16
    raise KeyError(canvas)


@functools.lru_cache(maxsize=None)
def batch(canvas, n):
    """-> (x [n, H, W, 3], hw [n, 2]) of the first n images of a canvas"""
    from isegmi.maskrcnn import prepare_images
    ims, div = images(canvas)
    x, hw = ims if isinstance(ims, tuple) else prepare_images(ims[:n], div)
    x, hw = x[:n], hw[:n]
    assert x.shape[0] == n, (canvas, n)
    return x, hw


# ---- models: name -> (class, state dict, config); the state dicts are built once per process
SEED = 5   # tests/test_fasterrcnn_gpu.py SEED_CLASSES: R-50 weights that give detections on the 128 x 160 canvas


@functools.lru_cache(maxsize=None)
def model_parts(name):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import maskrcnn_c4_state_dict, maskrcnn_state_dict
    if name == "r50":
        return MaskRCNN, maskrcnn_state_dict(SEED), MaskRCNNConfig()
    if name == "agnostic":
        return (MaskRCNN, maskrcnn_state_dict(SEED, mask=False, num_classes=9, cls_agnostic=True),
                dataclasses.replace(MaskRCNNConfig(), MASK_ON=False, NUM_CLASSES=9, CLS_AGNOSTIC_BBOX_REG=True))
    if name == "gn":
        import maskrcnn_gn_common as gc
        return MaskRCNN, gc.state_dict(), gc.gn_cfg()
    if name == "keypoint":
        from test_keypointrcnn_gpu import _cfg, _sd
        return MaskRCNN, _sd(), _cfg()
    if name == "c4":
        return MaskRCNN, maskrcnn_c4_state_dict(1234), dataclasses.replace(MaskRCNNConfig.c4(), RPN_POST_NMS_TOP_N_TEST=100)
    if name == "x50":
        import resnext_ref as xr
        return MaskRCNN, xr.state_dict(), xr.config()
    if name == "retinanet":
        import retinanet_common as rc
        from isegmi.retinanet import RetinaNet, RetinaNetConfig
        return RetinaNet, rc.state_dict(), RetinaNetConfig()
    raise KeyError(name)


def _f(name, model="r50", batch=1, canvases=("tiny",), fp16=False, **params):
    return dict(name=name, model=model, batch=batch, canvases=tuple(canvases), fp16=fp16, params=params)


# One form per branch the graph code takes.  `canvases` is the sequence of forwards of one run (the engine is built for the first, the largest);
# `params` are engine parameters set before the first forward.
FORMS = [
    _f("fpn_bs1"), _f("fpn_bs2", batch=2),
    _f("fpn_conv_groups0_bs1", conv_groups=0), _f("fpn_conv_groups0_bs2", batch=2, conv_groups=0),
    _f("fpn_select_groups0_bs1", rpn_select_groups=0), _f("fpn_select_groups0_bs2", batch=2, rpn_select_groups=0),
    _f("fpn_select_groups0_on_tail1_bs1", rpn_select_groups=0, rpn_select_on_tail=1),
    _f("fpn_select_groups0_on_tail0_bs2", batch=2, rpn_select_groups=0, rpn_select_on_tail=0),
    _f("fpn_multi_stream0", batch=2, multi_stream=0),
    _f("fpn_roi_table0", batch=2, roi_table=0), _f("fpn_roi_table3", batch=2, roi_table=3),
    _f("fpn_box_nms_chip_wide0", batch=2, box_nms_chip_wide=0),
    _f("fpn_roi_aligned1", batch=2, roi_aligned=1),
    _f("fpn_graph", batch=2, canvases=("tiny", "tiny", "tiny"), graph=1),
    _f("fpn_two_canvases", batch=2, canvases=("tiny", "tiny_b", "tiny")),
    _f("fpn_detections_cap", batch=2, detections_cap=128),
    _f("fpn_fp16_bs2", batch=2, fp16=True),
    _f("gn", model="gn", batch=2, canvases=("small",)),
    _f("mask_on0", batch=2, mask_on=0),
    _f("keypoint_on1", model="keypoint", batch=2, canvases=("kp",)),
    _f("cls_agnostic1", model="agnostic"),
    _f("c4_mask", model="c4", canvases=("c4",)), _f("c4_box_only", model="c4", canvases=("c4",), mask_on=0),
    _f("x50_32x8d", model="x50", batch=2, canvases=("small",)),
    _f("retinanet", model="retinanet", batch=2, canvases=("small", "tiny", "small")),
]

BUFFERS = (["proposals", "roi_order", "box.roi_table", "mask.roi_table", "kp.roi_table"] + ["anchors.%d" % l for l in range(5)] +
           ["det.count", "det.box", "det.score", "det.label", "det.mask28", "det.mask14", "det.kpt", "det.kscore"] +
           ["P%d" % l for l in range(2, 8)] + ["fpn.last%d" % l for l in range(1, 5)])
DET_ROWS = ("det.box", "det.score", "det.label", "det.mask28", "det.mask14", "det.kpt", "det.kscore")
DTYPES = ("f32", "i32", "u8", "i64", "f16")
TRACE_TAG = "convlaunch\t"   # what every conv_trace line starts with; the records hold the rest


def _key(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:8]


def pack(recorded_at, hash_dropped, forms):
    """The manifest file's form: a forward's conv launch lines and a form's buffer table are stored once, under a key of their content, and the forms
    name the keys (most forms share them).  -> text, one line per entry"""
    traces, tables, out = {}, {}, {}
    for name, rec in forms.items():
        rec = dict(rec)
        for t in rec["conv_trace"]:
            traces[_key(t)] = t
        tables[_key(rec["buffers"])] = rec["buffers"]
        rec["conv_trace"], rec["buffers"] = [_key(t) for t in rec["conv_trace"]], _key(rec["buffers"])
        out[name] = rec
    dump = lambda d: "{\n" + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True)) for k in sorted(d)) + "\n }"
    return ('{\n "recorded_at": %s,\n "hash_dropped": %s,\n "forms": %s,\n "buffer_tables": %s,\n "conv_traces": %s\n}\n'
            % (json.dumps(recorded_at), json.dumps(hash_dropped), dump(out), dump(tables), dump(traces)))


def unpack(manifest, name):
    """-> the record of one form as run_form returns it"""
    rec = dict(manifest["forms"][name])
    rec["conv_trace"] = [manifest["conv_traces"][k] for k in rec["conv_trace"]]
    rec["buffers"] = manifest["buffer_tables"][rec["buffers"]]
    return rec


def _buffer_info(m, name):
    from isegmi import _ffi
    nb = C.c_int64(); dt = C.c_int32(); nd = C.c_int32(); shp = (C.c_int64 * 4)()
    if _ffi.lib().isegmi_engine_buffer_info(m._h, name.encode(), None, C.byref(nb), C.byref(dt), shp, C.byref(nd)) != 0:
        return "absent"
    return dict(bytes=int(nb.value), dtype=DTYPES[dt.value], shape=[int(shp[i]) for i in range(nd.value)])


def _op_stats(m):
    """-> {label: [summed algorithmic bytes, scopes]}; clears the engine's accumulators"""
    from isegmi import _ffi
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    _ffi.check(_ffi.lib().isegmi_engine_op_stats(m._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    labels = names.value.decode().split("\n") if cnt.value else []
    return {labels[i]: [float(by[i]), int(ln[i])] for i in range(cnt.value)}


def _conv_stats(m):
    from isegmi import _ffi
    f, ms, n = C.c_double(), C.c_double(), C.c_int64()
    _ffi.check(_ffi.lib().isegmi_engine_conv_stats(m._h, C.byref(f), C.byref(ms), C.byref(n)))
    return dict(launches=int(n.value), flops=float(f.value))


def _graph_stats(m):
    from isegmi import _ffi
    cap, rep, fail = C.c_int64(), C.c_int64(), C.c_int64()
    _ffi.check(_ffi.lib().isegmi_engine_graph_stats(m._h, C.byref(cap), C.byref(rep), C.byref(fail)))
    return dict(captures=int(cap.value), replays=int(rep.value), failures=int(fail.value))


def _det_hash(m, n):
    """-> (sha256 over det.count and the first count rows per image of every det.* result buffer that exists, the counts)"""
    cnt = m.fetch("det.count", n)
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(cnt).tobytes())
    for k in DET_ROWS:
        if _buffer_info(m, k) == "absent":
            continue
        a = m.fetch(k, n)
        for i in range(n):
            h.update(k.encode()); h.update(np.ascontiguousarray(a[i, : cnt[i]]).tobytes())
    return h.hexdigest(), [int(c) for c in cnt]


def _forwards(m, form):
    """One run of the form's canvas sequence -> per step (detection hash, counts)"""
    out = []
    for canvas in form["canvases"]:
        x, hw = batch(canvas, form["batch"])
        n = m.upload(x, hw)
        m.forward_device(n); m.sync()
        out.append(_det_hash(m, n))
    return out


def run_form(form, stderr_begin, stderr_end):
    """Builds the form's engine and runs it: the canvas sequence twice without instrumentation (detection hashes of both runs), then once under
    timing / op_timing / conv_timing / conv_trace.  stderr_begin() starts a capture of file descriptor 2, stderr_end() -> the text written since.
    -> the form's record"""
    from isegmi import _ffi
    cls, sd, cfg = model_parts(form["model"])
    x0 = batch(form["canvases"][0], form["batch"])[0]
    kw = dict(fp16=True) if form["fp16"] else {}
    m = cls(sd, x0.shape[1], x0.shape[2], cfg=cfg, max_batch=form["batch"], **kw)
    try:
        for k, v in form["params"].items():
            m.set_param(k, float(v))
        first, second = _forwards(m, form), _forwards(m, form)
        rec = dict(counts=[c for _, c in first], hash=[h for h, _ in first], hash_repeat=[h for h, _ in second])
        if form["params"].get("graph"):
            rec["graph_stats"] = _graph_stats(m)
        for k in ("timing", "op_timing", "conv_timing", "conv_trace"):
            m.set_param(k, 1.0)
        _op_stats(m); _conv_stats(m)
        rec["marks"], rec["conv_trace"] = [], []
        for canvas in form["canvases"]:
            x, hw = batch(canvas, form["batch"])
            n = m.upload(x, hw)
            stderr_begin()
            try:
                m.forward_device(n); m.sync()
            finally:
                err = stderr_end()
            rec["marks"].append([name for name, _ in m.timings()])
            rec["conv_trace"].append([ln[len(TRACE_TAG):] for ln in err.splitlines() if ln.startswith(TRACE_TAG)])
        if not form["model"] == "c4":   # the C4 graph may gain the shared stages' scopes: instrumentation only
            rec["op_stats"] = _op_stats(m)
        rec["conv_stats"] = _conv_stats(m)
        wb, bb = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_memory(m._h, C.byref(wb), C.byref(bb)))
        rec["memory"] = dict(weight_bytes=int(wb.value), buffer_bytes=int(bb.value))
        rec["buffers"] = {k: _buffer_info(m, k) for k in BUFFERS}
        return rec
    finally:
        m.close()
