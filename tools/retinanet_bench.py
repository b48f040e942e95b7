#!/usr/bin/env python3
"""RetinaNet R-50-FPN throughput at the 800 x 1344 canvas, bs = 2 and bs = 1, seeded random weights.  Per batch size: images/s over back-to-back
forwards on a resident batch, p50 step latency from the engine's completion marks, the convolutions' FLOPs and fraction of the fp32 MFMA peak (conv_timing
pass), the tail's two stages from the engine's op stats (op_timing pass: HIP-event time and algorithmic bytes) -- the selection's achieved bytes/s also as a
fraction of the same run's isegmi_box_calibrate copy rate -- and, next to it, Mask R-CNN R-50-FPN forwards on the same box, canvas and batch.

    python tools/retinanet_bench.py [--steps 20] [--warmup 3] [--out profiles/retinanet_bench.json]
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

PEAK_F32_MFMA_TFLOPS = 157.3
H, W = 800, 1344


def conv_stats(net):
    from isegmi import _ffi
    f, ms, n = C.c_double(), C.c_double(), C.c_int64()
    _ffi.check(_ffi.lib().isegmi_engine_conv_stats(net._h, C.byref(f), C.byref(ms), C.byref(n)))
    return f.value, ms.value, n.value


def op_stats(net):
    from isegmi import _ffi
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    _ffi.check(_ffi.lib().isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    labels = names.value.decode().split("\n") if cnt.value else []
    return [(labels[i], float(us[i]), float(by[i]), int(ln[i])) for i in range(cnt.value)]


def timed(net, bs, steps, warmup):
    """-> (images/s, p50 step ms) of `steps` forwards enqueued back to back on the resident batch."""
    for _ in range(warmup):
        net.forward_device(bs)
    net.sync()
    net.step_times()
    t0 = time.perf_counter()
    net.mark_step()
    for _ in range(steps):
        net.forward_device(bs)
        net.mark_step()
    net.sync()
    dt = (time.perf_counter() - t0) / steps
    ms = sorted(net.step_times())
    return bs / dt, (ms[len(ms) // 2] if ms else None)


def run(bs, steps, warmup, box):
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.retinanet import RetinaNet
    from isegmi.weights import maskrcnn_state_dict, retinanet_state_dict
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(bs)]
    net = RetinaNet(retinanet_state_dict(1234), H, W, max_batch=bs)
    net.upload_u8(imgs)
    ips, p50 = timed(net, bs, steps, warmup)
    dets = net.fetch("det.count", bs).tolist()
    sel = net.fetch("retina.sel_cnt", bs).tolist()
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
                         "achieved_gbs": None if gbs is None else round(gbs, 1),
                         "fraction_of_copy_rate": None if gbs is None else round(gbs / box["hbm_copy_gbs"], 4)}
    mr = MaskRCNN(maskrcnn_state_dict(1234), H, W, max_batch=bs)
    mr.upload_u8(imgs)
    mips, mp50 = timed(mr, bs, steps, warmup)
    mr.close()
    return {"batch": bs, "canvas": [H, W], "images_per_s": round(ips, 2), "p50_step_ms": None if p50 is None else round(p50, 3),
            "detections": dets, "selected_per_level": sel,
            "conv_gflop_per_step": round(flops / steps / 1e9, 1), "conv_ms_per_step": round(cms / steps, 3), "conv_launches_per_step": launches // steps,
            "conv_tflops": round(conv_tf, 2), "conv_mfma_fraction": round(conv_tf / PEAK_F32_MFMA_TFLOPS, 3),
            "stages": stages,
            "maskrcnn_r50_fpn_same_box": {"images_per_s": round(mips, 2), "p50_step_ms": None if mp50 is None else round(mp50, 3), "note": "forward only, no paste"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retinanet_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    from isegmi.retinanet import retina_level_shapes
    _ffi.set_device(0)
    box = _ffi.box_calibrate()
    floor = sum(h * w for h, w in retina_level_shapes(H, W)) * 9 * 80 * 4   # every class logit once
    res = {"model": "retinanet_R-50-FPN", "weights": "random (seed 1234)", "box": box, "select_logit_bytes_per_image": floor,
           "runs": [run(bs, a.steps, a.warmup, box) for bs in (2, 1)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
