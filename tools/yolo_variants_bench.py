#!/usr/bin/env python3
"""YOLOv3-SPP and YOLOv3-tiny throughput on seeded random weights, next to yolov3 in the same run, at 416 x 416 bs = 8 and bs = 1 and at
608 x 608 bs = 1: images/s over back-to-back forwards on a resident batch (the median of three windows; all three are recorded), p50 step latency from the engine's completion marks, the convolutions' time and the
HBM-bound stages from the engine's op stats (tools/yolov3_bench.py's run()), and the same run's isegmi_box_calibrate.

spp_concat is also timed alone at 13 x 13 x 512 and 19 x 19 x 512 (the stride-32 maps of 416 and 608), bs = 1 and 8, between HIP events, against
  - three isegmi_op_maxpool launches (13, 9, 5) on the same input: a LOWER bound of the unfused form, which also needs the concat;
  - its byte floor, 5 C floats per pixel (C read, 4 C written), at the calibrated copy rate;
  - a device-to-device copy of the same bytes.

    python tools/yolo_variants_bench.py [--steps 100] [--warmup 3] [--out profiles/yolo_variants_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from retinanet_bench import conv_stats, op_stats, timed  # noqa: E402
from yolov3_bench import RUNS, Events  # noqa: E402

VARIANTS = ("yolov3", "spp", "tiny")
SPP_ALONE = ((13, 1), (13, 8), (19, 1), (19, 8))   # (map side, batch) at C = 512


def run(variant, size, bs, steps, warmup, sd):
    import dataclasses
    from isegmi.yolov3 import YoloV3, YoloV3Config
    cfg = YoloV3Config.tiny() if variant == "tiny" else YoloV3Config(variant=variant)
    net = YoloV3(sd, size, size, dataclasses.replace(cfg, height=size, width=size), max_batch=bs)
    net.upload(np.random.default_rng(0).uniform(0, 1, (bs, size, size, 3)).astype(np.float32))
    samples = [timed(net, bs, steps, warmup) for _ in range(3)]   # the spread of the same command on the same code
    ips, p50 = sorted(samples)[1]
    dets = net.fetch("det.count", bs).tolist()
    total = net.candidate_counts(bs)[1].tolist()
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
    stages = {label: {"us_per_step": round(us / steps, 1), "bytes_per_step": int(by / steps), "launch_groups_per_step": ln // steps} for label, us, by, ln in ops}
    return {"variant": variant, "batch": bs, "canvas": [size, size], "images_per_s": round(ips, 2), "p50_step_ms": None if p50 is None else round(p50, 3),
            "images_per_s_samples": [round(v, 2) for v, _ in samples],
            "detections": dets, "candidates_before_cut_per_level": total, "conv_gflop_per_step": round(flops / steps / 1e9, 1),
            "conv_ms_per_step": round(cms / steps, 3), "conv_launches_per_step": launches // steps, "stages": stages}


def spp_alone(side, bs, reps, ev, box, Cc=512):
    from isegmi import _ffi
    x = _ffi.DeviceBuffer.from_numpy(np.random.default_rng(side + bs).normal(0, 1, (bs, side, side, Cc)).astype(np.float32))
    out = _ffi.DeviceBuffer((bs, side, side, 4 * Cc))
    pools = [_ffi.DeviceBuffer((bs, side, side, Cc)) for _ in range(3)]
    nbytes = 5 * x.nbytes
    src, dst = _ffi.DeviceBuffer((nbytes,), np.uint8), _ffi.DeviceBuffer((nbytes,), np.uint8)
    src.zero()
    lib = _ffi.lib()

    def fused(zp):
        return lambda: _ffi.check(lib.isegmi_op_spp_concat(x.ptr, bs, side, side, Cc, zp, out.ptr, None))

    def three():
        for k, o in zip((13, 9, 5), pools):
            _ffi.check(lib.isegmi_op_maxpool(x.ptr, bs, side, side, Cc, k, 1, k // 2, o.ptr, None))

    def copy():
        assert ev.hip.hipMemcpyAsync(dst.ptr, src.ptr, C.c_size_t(nbytes), 3, None) == 0   # hipMemcpyDeviceToDevice
    # three samples of each, interleaved, so that a drift of the clock shows as spread and not as a difference between the forms
    t = {"spp_concat": [], "spp_concat_zero_pad": [], "three_maxpool": [], "copy": []}
    for _ in range(3):
        t["spp_concat"].append(ev.time_us(fused(0), reps)); t["three_maxpool"].append(ev.time_us(three, reps))
        t["spp_concat_zero_pad"].append(ev.time_us(fused(1), reps)); t["copy"].append(ev.time_us(copy, reps))
    med = {k: sorted(v)[1] for k, v in t.items()}
    floor_us = nbytes / (box["hbm_copy_gbs"] * 1e3)
    return {"map": [side, side], "channels": Cc, "batch": bs, "bytes_5c": nbytes, "reps_per_sample": reps,
            "us_samples": {k: [round(u, 2) for u in v] for k, v in t.items()}, "spp_concat_us": round(med["spp_concat"], 2),
            "spp_concat_zero_pad_us": round(med["spp_concat_zero_pad"], 2), "three_maxpool_launches_us": round(med["three_maxpool"], 2),
            "d2d_copy_same_bytes_us": round(med["copy"], 2), "byte_floor_at_calibrated_copy_rate_us": round(floor_us, 2),
            "three_maxpool_over_spp_concat": round(med["three_maxpool"] / med["spp_concat"], 2), "spp_concat_over_copy": round(med["spp_concat"] / med["copy"], 2),
            "spp_concat_achieved_gbs": round(nbytes / med["spp_concat"] / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_variants_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    from isegmi.weights import yolov3_state_dict
    _ffi.set_device(0)
    box = _ffi.box_calibrate()
    t0 = time.time()
    res = {"models": "yolov3, yolov3-spp, yolov3-tiny (COCO-80)", "weights": "random (seed 1234)", "box": box, "runs": []}
    for variant in VARIANTS:
        sd = yolov3_state_dict(1234, variant=variant)
        res["runs"] += [run(variant, size, bs, a.steps, a.warmup, sd) for size, bs in RUNS]
    ev = Events()
    res["spp_concat_alone"] = [spp_alone(side, bs, 1000, ev, box) for side, bs in SPP_ALONE]
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
