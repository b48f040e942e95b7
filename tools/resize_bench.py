#!/usr/bin/env python3
"""The resize on the device against the resize on the host, one process, seeded random weights.  Every pair is measured ALTERNATELY
(host, device, host, device, ...) and reported as the median of --repeats rounds, with every sample kept:

  op_alone   isegmi_op_resample_u8 (fp32 epilogue, Mask R-CNN mean) at 480 x 640 -> 800 x 1067 and 3000 x 4000 -> 800 x 1067, bs 1 and 8, HIP-event
             time of `inner` back-to-back launches; its bytes (in + 12 out) per second next to the box calibration's copy rate
  pil        Image.resize on one host thread at the same shapes
  cocodemo   COCODemo.compute_prediction of one 480 x 640 image (Mask R-CNN R-50-FPN, bs = 1) in the two modes
  inference  inference() over 16 such images at bs = 8 in the two modes, with workers = 0 and the default 4
  detect_aug MaskRCNN.detect_aug on the shipped bbox-aug yaml (ten views) of one 480 x 640 image in the two modes

    python tools/resize_bench.py [--repeats 5] [--out profiles/resize_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

OUT_HW = (800, 1067)
SHAPES = ((480, 640), (3000, 4000))
PIXEL_MEAN = (102.9801, 115.9465, 122.7717)


def alternate(fns, repeats, warmup=1):
    """{name: fn} run in turn, `repeats` rounds -> {name: {"median_ms", "samples_ms"}}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 3), "samples_ms": [round(x, 3) for x in v]} for k, v in ts.items()}


def bench_op(repeats, calib):
    from isegmi import _ffi
    from isegmi.transforms import ResamplePlan
    L = _ffi.lib()
    oh, ow = OUT_HW
    Hp, Wp = -(-oh // 32) * 32, -(-ow // 32) * 32
    out = []
    for h, w in SHAPES:
        for bs in (1, 8):
            rng = np.random.default_rng(h + bs)
            ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(bs)]
            plan = ResamplePlan([(h, w)] * bs, [[(i, oh, ow, 0, 0, 0, i) for i in range(bs)]])
            blob = np.empty(plan.nbytes, np.uint8)
            plan.write(blob, ims)
            table = plan.header()[1][0]
            db, do = _ffi.DeviceBuffer.from_numpy(blob), _ffi.DeviceBuffer((bs, Hp, Wp, 3))
            m = (C.c_float * 3)(*PIXEL_MEAN); sd = (C.c_float * 3)(1.0, 1.0, 1.0)
            base = db.ptr.value
            inner = 10

            def run():
                for _ in range(inner):
                    _ffi.check(L.isegmi_op_resample_u8(C.c_void_p(base + plan.src_off), plan.pixel_bytes, C.c_void_p(base), table.ctypes.data_as(C.c_void_p), bs,
                                                       C.c_void_p(base + plan.coeff_off), plan.coeff_words, do.ptr, bs, Hp, Wp, Hp * Wp * 3, m, sd, 0, 0.0, None, 0, None))
                _ffi.sync()
            r = alternate({"op": run}, max(repeats, 7), 2)["op"]
            us = r["median_ms"] * 1e3 / inner
            nbytes = float(bs) * (h * w * 3 + 12.0 * Hp * Wp)
            row = {"op": "isegmi_op_resample_u8", "in": [h, w], "out": [oh, ow], "canvas": [Hp, Wp], "batch": bs, "us": round(us, 2),
                   "samples_us": [round(x * 1e3 / inner, 2) for x in r["samples_ms"]], "bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1),
                   "fraction_of_calibrated_copy": round(nbytes / us / 1e3 / calib["hbm_copy_gbs"], 4)}
            out.append(row)
            print(json.dumps(row), flush=True)
            db.free(); do.free()
    return out


def bench_pil(repeats):
    from PIL import Image
    out = []
    for h, w in SHAPES:
        im = Image.fromarray(np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8))
        r = alternate({"pil": lambda: im.resize((OUT_HW[1], OUT_HW[0]), Image.BILINEAR)}, max(repeats, 7), 2)["pil"]
        row = {"pil_resize": [h, w], "out": list(OUT_HW), "threads": 1, **r}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def images(n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(n)]


def bench_cocodemo_and_inference(repeats):
    from isegmi.predictor import COCODemo, inference
    from isegmi.weights import maskrcnn_state_dict
    demo = COCODemo(None, min_image_size=800, max_image_size=1333, confidence_threshold=0.5, state_dict=maskrcnn_state_dict(1234), max_batch=8)
    ims = images(16)
    res = {}
    try:
        def predict(mode):
            demo.resize = mode
            return demo.compute_prediction(ims[0])
        a, b = predict("host"), predict("device")
        res["cocodemo_bs1"] = {"image": [480, 640], "identical": bool(np.array_equal(a.bbox, b.bbox) and np.array_equal(a.get_field("mask"), b.get_field("mask"))),
                               **alternate({"host": lambda: predict("host"), "device": lambda: predict("device")}, repeats)}
        print(json.dumps(res["cocodemo_bs1"]), flush=True)
        for workers in (0, 4):
            same = json.dumps(inference(demo, ims, batch_size=8, workers=workers, resize="host")) == json.dumps(inference(demo, ims, batch_size=8, workers=workers, resize="device"))
            key = "inference_bs8_workers%d" % workers
            res[key] = {"images": 16, "identical": same,
                        **alternate({m: (lambda m=m: inference(demo, ims, batch_size=8, workers=workers, resize=m)) for m in ("host", "device")}, repeats)}
            print(json.dumps(res[key]), flush=True)
    finally:
        demo.resize = "host"
        demo.close()
    return res


def bench_detect_aug(repeats):
    from isegmi.config import cfg, to_bbox_aug_config
    from isegmi.maskrcnn import BBoxAugOverflow, MaskRCNN, bbox_aug_engine_side, bbox_aug_views
    from isegmi.weights import random_maskrcnn_state_dict
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml"))
    mc, aug = to_bbox_aug_config(c)
    ims = images(1, 5)
    side = bbox_aug_engine_side(mc, aug)
    net = MaskRCNN(random_maskrcnn_state_dict(mc, 1234), side, side, cfg=mc, max_batch=1)
    out = {"image": [480, 640], "views": [list(v) for v in bbox_aug_views((480, 640), mc, aug)]}
    try:
        net.reserve()
        for thr in (mc.ROI_SCORE_THRESH, 0.1, 0.2, 0.4):   # random weights score near-uniformly: the threshold under which ten views fit the pool
            net.set_param("roi_score_thresh", float(thr))
            try:
                a = net.detect_aug(ims, aug)
                break
            except BBoxAugOverflow:
                continue
        out["roi_score_thresh"] = float(thr)
        b = net.detect_aug(ims, aug, resize="device")
        out["identical"] = bool(np.array_equal(a[0].bbox, b[0].bbox) and np.array_equal(a[0].get_field("scores"), b[0].get_field("scores")))
        out.update(alternate({m: (lambda m=m: net.detect_aug(ims, aug, resize=m)) for m in ("host", "device")}, repeats))
    finally:
        net.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    calib = _ffi.box_calibrate()
    report = {"weights": "random (seed 1234)", "repeats": a.repeats, "box_calibration": calib, "host_cpus_used_by_pil": 1}
    report["op_alone"] = bench_op(a.repeats, calib)
    report["pil"] = bench_pil(a.repeats)
    report.update(bench_cocodemo_and_inference(a.repeats))
    report["detect_aug"] = bench_detect_aug(a.repeats)
    report["box_calibration_after"] = _ffi.box_calibrate()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
