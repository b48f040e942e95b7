"""Painter measurements: COCODemo.run_on_opencv_image with render="host" and render="device" on one Mask R-CNN R-50-FPN predictor
(800 x 1333 image, seeded random weights, confidence thresholds placed so that about 10 and about 100 detections are drawn), the same pair for Yolact
at 550 x 550, batch 8 (cli._overlay of postprocess() against isegmi.yolact.render_images), and isegmi_op_paint alone at D = 10 and 100 on 800 x 1333
planes with its bytes per second next to the box calibration's copy rate.  Medians over --rounds calls after --warmup calls.

    python tools/render_bench.py [--rounds 7] [--warmup 2] [--out profiles/render_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "instancesegmentation-jittor_amd")]


def median_s(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def bench_maskrcnn(rounds, warmup):
    from isegmi.predictor import COCODemo
    from isegmi.weights import maskrcnn_state_dict
    image = np.random.default_rng(0).integers(0, 256, (800, 1333, 3)).astype(np.uint8)
    demo = COCODemo(None, min_image_size=800, max_image_size=1333, confidence_threshold=-1.0, state_dict=maskrcnn_state_dict(1234), max_batch=1)
    out = []
    try:
        scores = np.sort(demo.compute_prediction(image).get_field("scores"))[::-1]
        for want in (10, 100):
            n = min(want, len(scores))
            demo.confidence_threshold = -1.0 if n == len(scores) else float((scores[n - 1] + scores[n]) / 2)
            drawn = len(demo.select_top_predictions(demo.compute_prediction(image)))
            r = {"model": "mask_rcnn_R_50_FPN", "image": [800, 1333], "detections_drawn": drawn}
            imgs = {}
            for render in ("host", "device"):
                demo.render = render
                r[render + "_ms"] = median_s(lambda: imgs.__setitem__(render, demo.run_on_opencv_image(image)), rounds, warmup) * 1e3
            demo.render = "host"
            r["identical"] = bool(np.array_equal(imgs["host"], imgs["device"]))
            r["speedup"] = r["host_ms"] / r["device_ms"]
            out.append(r)
            print(json.dumps(r), flush=True)
    finally:
        demo.close()
    return out


def bench_yolact(rounds, warmup):
    from isegmi.cli import _overlay
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, postprocess, render_images
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (550, 550, 3)).astype(np.uint8) for _ in range(8)]
    net = Yolact(yolact_state_dict(1234), max_batch=8)
    out = []
    try:
        for thr, top_k in ((0.15, 15), (0.0, None)):
            def host():
                o = net(frames)
                res = []
                for i, f in enumerate(frames):
                    classes, _, boxes, masks = postprocess(o, 550, 550, i, thr)
                    res.append(_overlay(f, masks[:top_k], boxes[:top_k], classes[:top_k]))
                return res
            a, b = host(), render_images(net, frames, thr, top_k)
            o = net(frames)
            drawn = sum(len(postprocess(o, 550, 550, i, thr)[0][:top_k]) for i in range(8))
            r = {"model": "yolact_resnet50", "batch": 8, "image": [550, 550], "score_threshold": thr, "top_k": top_k, "detections_drawn": drawn,
                 "host_ms": median_s(host, rounds, warmup) * 1e3, "device_ms": median_s(lambda: render_images(net, frames, thr, top_k), rounds, warmup) * 1e3,
                 "identical": bool(all(np.array_equal(x, y) for x, y in zip(a, b)))}
            r["speedup"] = r["host_ms"] / r["device_ms"]
            out.append(r)
            print(json.dumps(r), flush=True)
    finally:
        net.close()
    return out


def bench_op(rounds, calib):
    """isegmi_op_paint alone (it reads its lists back and checks them before the launch: that round trip is inside the time)"""
    from isegmi import _ffi
    H, W, slots = 800, 1333, 100
    rng = np.random.default_rng(2)
    L = _ffi.lib()
    img = _ffi.DeviceBuffer.from_numpy(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)); dst = _ffi.DeviceBuffer((H, W, 3), np.uint8)
    masks = _ffi.DeviceBuffer.from_numpy((rng.integers(0, 5, (slots, H, W), dtype=np.uint8) == 0).astype(np.uint8))   # a fifth of the pixels set
    out = []
    for D in (10, 100):
        e = np.zeros((D, 8), np.int32)
        e[:, 0] = np.arange(D); e[:, 1] = rng.integers(0, W // 2, D); e[:, 2] = rng.integers(0, H // 2, D)
        e[:, 3] = e[:, 1] + W // 3; e[:, 4] = e[:, 2] + H // 3; e[:, 5] = rng.integers(0, 1 << 24, D); e[:, 6] = 1
        de = _ffi.DeviceBuffer.from_numpy(e)
        inner = 10

        def run():
            for _ in range(inner):
                _ffi.check(L.isegmi_op_paint(img.ptr, H, W, masks.ptr, slots, H, W, de.ptr, D, None, 0, dst.ptr, None))
            _ffi.sync()
        s = median_s(run, rounds, 2) / inner
        nbytes = float(D) * H * W + 6.0 * H * W
        r = {"op": "isegmi_op_paint", "image": [H, W], "D": D, "us": s * 1e6, "gb_per_s": nbytes / s / 1e9, "fraction_of_calibrated_copy": nbytes / s / 1e9 / calib["hbm_copy_gbs"]}
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    calib = _ffi.box_calibrate()
    report = {"box_calibration": calib, "rounds": a.rounds, "warmup": a.warmup}
    report["op_alone"] = bench_op(max(a.rounds, 10), calib)
    report["maskrcnn"] = bench_maskrcnn(a.rounds, a.warmup)
    report["yolact"] = bench_yolact(a.rounds, a.warmup)
    report["box_calibration_after"] = _ffi.box_calibrate()
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("box calibration before / after:", calib, report["box_calibration_after"])


if __name__ == "__main__":
    main()
