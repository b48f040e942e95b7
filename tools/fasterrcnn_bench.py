#!/usr/bin/env python3
"""Faster R-CNN against Mask R-CNN on the same weights, box and process: R-50-FPN and R-50-C4 at the 800 x 1344 canvas, bs = 2 and bs = 1,
seeded random weights.  The box-only engine (MASK_ON False) and the mask engine are built side by side and measured ALTERNATELY, `--repeats` times each, so
the run's own spread stands next to the difference: images/s over back-to-back forwards on a resident batch and p50 step latency from the engine's completion
marks per repeat, launches per step (convolution launches + launch groups of the other stages), reserve() bytes and record-block bytes per step.

    python tools/fasterrcnn_bench.py [--steps 20] [--warmup 3] [--repeats 3] [--out profiles/fasterrcnn_bench.json]
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

H, W = 800, 1344


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


def launches(net, bs):
    from isegmi import _ffi
    L = _ffi.lib()
    f, ms, nconv = C.c_double(), C.c_double(), C.c_int64()
    net.set_param("conv_timing", 1.0)
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_conv_stats(net._h, C.byref(f), C.byref(ms), C.byref(nconv)))
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_conv_stats(net._h, C.byref(f), C.byref(ms), C.byref(nconv)))
    net.set_param("conv_timing", 0.0)
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    net.set_param("op_timing", 1.0)
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    net.set_param("op_timing", 0.0)
    return {"conv_launches": int(nconv.value), "other_launch_groups": sum(int(ln[i]) for i in range(cnt.value))}


def run(body, bs, steps, warmup, repeats):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import random_maskrcnn_state_dict
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(bs)]
    base = MaskRCNNConfig.c4() if body == "R-50-C4" else MaskRCNNConfig()
    nets, out = {}, {}
    for name, cfg in (("box_only", dataclasses.replace(base, MASK_ON=False)), ("mask", base)):
        net = MaskRCNN(random_maskrcnn_state_dict(cfg, 1234), H, W, cfg=cfg, max_batch=bs)
        wb, ab = net.reserve()
        net.upload_u8(imgs)
        nets[name] = net
        out[name] = {"reserve_weight_bytes": int(wb), "reserve_activation_bytes": int(ab), "record_block_bytes_per_step": int(net.coco_record_bytes(bs)[0]),
                     "images_per_s": [], "p50_step_ms": []}
    for _ in range(repeats):                      # alternated: drift of the box lands on both engines alike
        for name in ("box_only", "mask"):
            ips, p50 = timed(nets[name], bs, steps, warmup)
            out[name]["images_per_s"].append(round(ips, 2))
            out[name]["p50_step_ms"].append(None if p50 is None else round(p50, 3))
    for name, net in nets.items():
        out[name].update(launches(net, bs))
        out[name]["detections"] = net.fetch("det.count", bs).tolist()
        net.close()
    b, m = out["box_only"]["images_per_s"], out["mask"]["images_per_s"]
    spread = max(max(b) - min(b), max(m) - min(m))
    out.update(body=body, batch=bs, canvas=[H, W], spread_images_per_s=round(spread, 2),
               box_only_minus_mask_images_per_s=round(float(np.median(b) - np.median(m)), 2),
               box_only_not_slower_beyond_spread=bool(np.median(b) >= np.median(m) - spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bodies", nargs="+", default=["R-50-FPN", "R-50-C4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasterrcnn_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    res = {"weights": "random (seed 1234)", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "note": "forward only on a resident batch; the mask engine's paste / RLE stage is not in these numbers",
           "runs": [run(body, bs, a.steps, a.warmup, a.repeats) for body in a.bodies for bs in (2, 1)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
