#!/usr/bin/env python3
"""YOLOv3 throughput on seeded random weights at 416 x 416 bs = 8 and bs = 1 and at 608 x 608 bs = 1.  Per run: images/s over back-to-back forwards
on a resident batch, p50 step latency from the engine's completion marks, the convolutions' FLOPs and fraction of the fp32 MFMA peak of the same run's
isegmi_box_calibrate (conv_timing pass), the tail's stages from the engine's op stats (op_timing pass: HIP-event time and algorithmic bytes).

Random weights pass far more anchors than a trained model does, so yolo_select is also timed alone on a second input: head tensors drawn so that about 0.1 %
of the anchors pass the objectness test at 0.5.  Its time stands against its byte floor -- the head tensors once, N * sum(H_l W_l) * A * (5 + C) * 4 bytes -- and
against a device-to-device copy of the same bytes, both between HIP events in the same run.

    python tools/yolov3_bench.py [--steps 20] [--warmup 3] [--out profiles/yolov3_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from retinanet_bench import conv_stats, op_stats, timed  # noqa: E402

RUNS = ((416, 8), (416, 1), (608, 1))


def run(size, bs, steps, warmup, box, sd):
    from isegmi.yolov3 import YoloV3, YoloV3Config
    rng = np.random.default_rng(0)
    net = YoloV3(sd, size, size, YoloV3Config(), max_batch=bs)
    net.upload(rng.uniform(0, 1, (bs, size, size, 3)).astype(np.float32))
    ips, p50 = timed(net, bs, steps, warmup)
    dets = net.fetch("det.count", bs).tolist()
    kept, total = (a.tolist() for a in net.candidate_counts(bs))
    net.set_param("conv_timing", 1.0)
    net.forward_device(bs); net.sync(); conv_stats(net)
    for _ in range(steps):
        net.forward_device(bs)
    net.sync()
    flops, cms, launches = conv_stats(net)
    net.set_param("conv_timing", 0.0)
    net.set_param("op_timing", 1.0)
    net.forward_device(bs); net.sync(); op_stats(net)
    for _ in range(steps):
        net.forward_device(bs)
    net.sync()
    ops = op_stats(net)
    net.close()
    conv_tf = flops / (cms * 1e-3) / 1e12 if cms > 0 else 0.0
    stages = {}
    for label, us, by, ln in ops:
        gbs = by / us / 1e3 if us > 0 else None
        stages[label] = {"us_per_step": round(us / steps, 1), "bytes_per_step": int(by / steps), "launch_groups_per_step": ln // steps,
                         "achieved_gbs": None if gbs is None else round(gbs, 1)}
    return {"batch": bs, "canvas": [size, size], "images_per_s": round(ips, 2), "p50_step_ms": None if p50 is None else round(p50, 3),
            "detections": dets, "candidates_kept_per_level": kept, "candidates_before_cut_per_level": total,
            "conv_gflop_per_step": round(flops / steps / 1e9, 1), "conv_ms_per_step": round(cms / steps, 3), "conv_launches_per_step": launches // steps,
            "conv_tflops": round(conv_tf, 2), "conv_mfma_fraction_of_calibrated_peak": round(conv_tf / box["mfma_f32_tflops"], 3), "stages": stages}


class Events:
    """HIP events on the null stream, through the runtime libisegmi.so already loaded."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time_us(self, enqueue, reps):
        """Device time of one of `reps` back-to-back enqueue() calls."""
        enqueue()
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(reps):
            enqueue()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3 / reps


def sparse_select(size, bs, reps, ev, pass_fraction=0.001):
    """yolo_select alone on heads whose objectness logits are N(mu, 1) with P(logit > 0) = pass_fraction (conf_thresh 0.5), class logits N(-2, 1.5)."""
    from statistics import NormalDist
    from isegmi import _ffi
    from isegmi.yolov3 import YoloV3Config, yolo_grids
    cfg = YoloV3Config()
    rng = np.random.default_rng(size + bs)
    mu = NormalDist().inv_cdf(pass_fraction)
    heads, passed, anchors = [], 0, 0
    for gh, gw in yolo_grids(size, size):
        h = rng.normal(0, 1.5, (bs, gh, gw, 3, 85)).astype(np.float32)
        h[..., 5:] -= np.float32(2.0)
        h[..., 4] = rng.normal(mu, 1.0, h.shape[:-1]).astype(np.float32)
        passed += int((h[..., 4] > 0).sum()); anchors += h[..., 4].size
        heads.append(h.reshape(bs, gh, gw, 255))
    dev = [_ffi.DeviceBuffer.from_numpy(h) for h in heads]
    nbytes = sum(d.nbytes for d in dev)
    ptrs = (C.c_void_p * 3)(*[d.ptr.value for d in dev])
    grid = (C.c_int32 * 6)(*[v for g in yolo_grids(size, size) for v in g])
    strides = (C.c_int32 * 3)(32, 16, 8)
    an = np.ascontiguousarray(cfg.level_anchors())
    top_n = cfg.pre_nms_top_n
    wsb = _ffi.lib().isegmi_op_yolo_select_workspace(3, bs, grid, 3, 80, top_n)
    ws = _ffi.DeviceBuffer((wsb,), np.uint8)
    ob, os_, ol = _ffi.DeviceBuffer((bs, 3 * top_n, 4)), _ffi.DeviceBuffer((bs, 3 * top_n)), _ffi.DeviceBuffer((bs, 3 * top_n), np.int32)
    oc, ot = _ffi.DeviceBuffer((bs, 3), np.int32), _ffi.DeviceBuffer((bs, 3), np.int32)

    def select():
        _ffi.check(_ffi.lib().isegmi_op_yolo_select(3, bs, ptrs, grid, strides, an.ctypes.data_as(C.c_void_p), 3, 80, top_n, cfg.conf_thresh, 1, 0.0, size, size,
                                                    ws.ptr, wsb, ob.ptr, os_.ptr, ol.ptr, oc.ptr, ot.ptr, None))
    src, dst = _ffi.DeviceBuffer((nbytes,), np.uint8), _ffi.DeviceBuffer((nbytes,), np.uint8)
    src.zero()

    def copy():
        assert ev.hip.hipMemcpyAsync(dst.ptr, src.ptr, C.c_size_t(nbytes), 3, None) == 0   # hipMemcpyDeviceToDevice
    sel_us, copy_us = ev.time_us(select, reps), ev.time_us(copy, reps)
    return {"batch": bs, "canvas": [size, size], "anchors": anchors, "anchors_passing_objectness": passed, "candidates_before_cut_per_level": ot.numpy().tolist(),
            "head_bytes": nbytes, "yolo_select_us": round(sel_us, 2), "d2d_copy_same_bytes_us": round(copy_us, 2), "select_over_copy": round(sel_us / copy_us, 2),
            "select_achieved_gbs_on_head_bytes": round(nbytes / sel_us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolov3_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    from isegmi.weights import yolov3_state_dict
    _ffi.set_device(0)
    box = _ffi.box_calibrate()
    sd = yolov3_state_dict(1234)
    t0 = time.time()
    res = {"model": "yolov3 (Darknet-53, COCO-80)", "weights": "random (seed 1234)", "box": box,
           "runs": [run(size, bs, a.steps, a.warmup, box, sd) for size, bs in RUNS]}
    ev = Events()
    res["sparse_select"] = [sparse_select(size, bs, 50, ev) for size, bs in RUNS]
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
