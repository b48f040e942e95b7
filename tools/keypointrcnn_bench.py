#!/usr/bin/env python3
"""Keypoint R-CNN against the box-only engine on the same trunk, box and process: R-50-FPN at the 800 x 1344 canvas, bs = 2 and bs = 1, seeded
random weights.  The keypoint engine (KEYPOINT_ON) and the two-class box-only engine are built side by side and measured ALTERNATELY, `--repeats` times each,
so the run's own spread stands next to the difference: images/s over back-to-back forwards on a resident batch and p50 step latency from the engine's
completion marks per repeat, launches per step, reserve() bytes and record-block bytes per step; from a conv_timing and an op_timing pass the keypoint
head's convolutions (the keypoint engine's convolution time and FLOPs minus the box-only engine's: the eight conv_fcn layers and the packed 3 x 3 -> 68 layer)
with their fraction of the fp32 MFMA peak, and the decode kernel's time with the mean resized map size of the run's detections and the positions it evaluates
per second.  The seeded two-class predictor gives one or two detections per image at upstream's SCORE_THRESH 0.05 (it keeps the 81-class background bias), so
the run lowers the threshold (`--score-thresh`, both engines alike) until the images are full: the head's convolutions cost the same either way, the decode
kernel's work is the detections'.  That two-class engine at the lowered threshold is not the work DESIGN.md 13 measured, so a THIRD engine -- Faster R-CNN as
there: 81 classes, SCORE_THRESH 0.05 -- is measured in the same alternation, and the one condition of this measurement is written into the json:
`box_only_not_below_design13` = its median images/s is not below the lowest repeat recorded in DESIGN.md 13 by more than this run's own spread.

    python tools/keypointrcnn_bench.py [--steps 20] [--warmup 3] [--repeats 3] [--out profiles/keypointrcnn_bench.json]
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
PEAK_F32_MFMA_TFLOPS = 157.3
DECODE_LABEL = "keypoint_decode"
DESIGN13_BOX_ONLY_IMAGES_PER_S = {2: 269.2, 1: 242.2}   # DESIGN.md 13, R-50-FPN box-only: the lowest of the recorded repeats at bs 2 / bs 1


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


def stage_stats(net, bs, steps):
    """conv_timing and op_timing passes of `steps` forwards each -> convolution launches, FLOPs and ms per step, the other stages' launch groups and us per step by label."""
    from isegmi import _ffi
    L = _ffi.lib()
    f, ms, nconv = C.c_double(), C.c_double(), C.c_int64()
    net.set_param("conv_timing", 1.0)
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_conv_stats(net._h, C.byref(f), C.byref(ms), C.byref(nconv)))
    for _ in range(steps):
        net.forward_device(bs)
    net.sync()
    _ffi.check(L.isegmi_engine_conv_stats(net._h, C.byref(f), C.byref(ms), C.byref(nconv)))
    net.set_param("conv_timing", 0.0)
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    net.set_param("op_timing", 1.0)
    net.forward_device(bs); net.sync()
    _ffi.check(L.isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    for _ in range(steps):
        net.forward_device(bs)
    net.sync()
    _ffi.check(L.isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    net.set_param("op_timing", 0.0)
    labels = names.value.decode().split("\n")
    ops = {labels[i]: {"us_per_step": us[i] / steps, "launch_groups_per_step": ln[i] / steps} for i in range(cnt.value)}
    return {"conv_launches": int(nconv.value) // steps, "conv_gflop_per_step": f.value / steps / 1e9, "conv_ms_per_step": ms.value / steps,
            "other_launch_groups": int(sum(o["launch_groups_per_step"] for o in ops.values())), "ops": ops}


def run(bs, steps, warmup, repeats, score_thresh):
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import random_maskrcnn_state_dict
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(bs)]
    box_cfg = dataclasses.replace(MaskRCNNConfig(), MASK_ON=False, NUM_CLASSES=2, ROI_SCORE_THRESH=score_thresh)
    nets, out = {}, {}
    names = ("keypoint", "box_only", "fasterrcnn_81")
    for name, cfg in zip(names, (dataclasses.replace(box_cfg, KEYPOINT_ON=True), box_cfg, dataclasses.replace(MaskRCNNConfig(), MASK_ON=False))):
        net = MaskRCNN(random_maskrcnn_state_dict(cfg, 1234), H, W, cfg=cfg, max_batch=bs)
        wb, ab = net.reserve()
        net.upload_u8(imgs)
        nets[name] = net
        out[name] = {"reserve_weight_bytes": int(wb), "reserve_activation_bytes": int(ab), "record_block_bytes_per_step": int(net.coco_record_bytes(bs)[0]),
                     "images_per_s": [], "p50_step_ms": []}
    for _ in range(repeats):                      # alternated: drift of the box lands on both engines alike
        for name in names:
            ips, p50 = timed(nets[name], bs, steps, warmup)
            out[name]["images_per_s"].append(round(ips, 2))
            out[name]["p50_step_ms"].append(None if p50 is None else round(p50, 3))
    for name, net in nets.items():
        out[name].update(stage_stats(net, bs, steps))
        out[name]["detections"] = net.fetch("det.count", bs).tolist()
    kp, bx = out["keypoint"], out["box_only"]
    same = all(np.array_equal(nets["keypoint"].fetch(k, bs), nets["box_only"].fetch(k, bs)) for k in ("det.count", "det.box", "det.score", "det.label"))
    cnt, box = nets["keypoint"].fetch("det.count", bs), nets["keypoint"].fetch("det.box", bs)
    live = np.concatenate([box[n, :cnt[n]] for n in range(bs)]) if cnt.sum() else np.zeros((0, 4), np.float32)
    area = np.ceil(np.maximum(live[:, 2] - live[:, 0], 1)) * np.ceil(np.maximum(live[:, 3] - live[:, 1], 1))
    gflop, ms = kp["conv_gflop_per_step"] - bx["conv_gflop_per_step"], kp["conv_ms_per_step"] - bx["conv_ms_per_step"]
    dec = [v for k, v in kp["ops"].items() if k.startswith(DECODE_LABEL)]
    dec_us = dec[0]["us_per_step"] if dec else None
    positions = float(area.sum()) * nets["keypoint"].cfg.NUM_KEYPOINTS
    out["keypoint_head"] = {
        "conv_launches": kp["conv_launches"] - bx["conv_launches"], "conv_gflop_per_step": round(gflop, 1), "conv_ms_per_step": round(ms, 3),
        "conv_tflops": round(gflop / ms, 2) if ms > 0 else None, "conv_frac_of_f32_mfma_peak": round(gflop / ms / PEAK_F32_MFMA_TFLOPS, 4) if ms > 0 else None,
        "decode_us_per_step": None if dec_us is None else round(dec_us, 1), "decode_detections": int(cnt.sum()),
        "decode_mean_wc_hc": round(float(area.mean()), 1) if len(area) else None,
        "decode_gpositions_per_s": round(positions / dec_us / 1e3, 2) if dec_us else None}
    for net in nets.values():
        net.close()
    spread = max(max(out[n]["images_per_s"]) - min(out[n]["images_per_s"]) for n in names)
    f81 = float(np.median(out["fasterrcnn_81"]["images_per_s"]))
    out.update(body="R-50-FPN", batch=bs, canvas=[H, W], score_thresh=score_thresh, box_path_identical=bool(same), spread_images_per_s=round(spread, 2),
               design13_box_only_images_per_s=DESIGN13_BOX_ONLY_IMAGES_PER_S[bs], box_only_not_below_design13=bool(f81 >= DESIGN13_BOX_ONLY_IMAGES_PER_S[bs] - spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--score-thresh", dest="score_thresh", type=float, default=0.012)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypointrcnn_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    res = {"weights": "random (seed 1234)", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "note": "forward only on a resident batch; box_only is the two-class Faster R-CNN on the keypoint engine's trunk weights at the lowered threshold, "
                   "fasterrcnn_81 the configuration DESIGN.md 13 measured (81 classes, SCORE_THRESH 0.05): the two are different work",
           "runs": [run(bs, a.steps, a.warmup, a.repeats, a.score_thresh) for bs in (2, 1)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
