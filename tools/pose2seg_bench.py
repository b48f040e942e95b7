#!/usr/bin/env python3
"""Pose2Seg throughput: images/s and person instances/s of isegmi.pose2seg.Pose2Seg.forward at the paper's widths (seeded synthetic weights),
bs images of 512 x 512 uint8 with a fixed number of persons each.  A step = upload of the images and keypoints, the whole forward and the
masks at every image's own size; steps are enqueued back to back (images and keypoints through pinned memory on the copy stream) and the
loop is synchronised at its end.  A second pass under the engine's conv_timing gives the convolutions' own time and FLOPs (HIP events per
launch) and their fraction of the fp32 MFMA peak.

    python tools/pose2seg_bench.py [--batch 8] [--persons 5] [--steps 20] [--warmup 3]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--persons", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from isegmi.pose2seg import Pose2Seg, Pose2SegConfig
    from isegmi.weights import pose2seg_state_dict
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (512, 512, 3), np.uint8) for _ in range(a.batch)]
    kps = []
    for _ in range(a.batch):
        k = np.zeros((a.persons, 17, 3), np.float32)
        k[..., 0] = rng.uniform(64, 448, (a.persons, 17)); k[..., 1] = rng.uniform(32, 480, (a.persons, 17)); k[..., 2] = 2
        kps.append(k)
    net = Pose2Seg(pose2seg_state_dict(1234), Pose2SegConfig(), max_batch=a.batch, max_instances=max(a.persons, 1))
    for _ in range(a.warmup):
        net.forward(imgs, kps)
    net.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        net.forward(imgs, kps)
    net.sync()
    dt = (time.perf_counter() - t0) / a.steps
    # a second pass under conv_timing: the engine's per-launch HIP-event times of the convolutions and their algorithmic FLOPs
    net.set_param("conv_timing", 1.0)
    net.conv_stats()
    for _ in range(a.steps):
        net.forward(imgs, kps)
    net.sync()
    flops, ms, launches = net.conv_stats()
    net.close()
    conv_tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    print(json.dumps({"model": "pose2seg", "batch": a.batch, "persons_per_image": a.persons, "ms_per_step": round(dt * 1e3, 3),
                      "images_per_s": round(a.batch / dt, 2), "instances_per_s": round(a.batch * a.persons / dt, 2),
                      "conv_gflop_per_step": round(flops / a.steps / 1e9, 2), "conv_ms_per_step": round(ms / a.steps, 3),
                      "conv_launches_per_step": launches // a.steps, "conv_tflops": round(conv_tf, 2),
                      "conv_mfma_fraction": round(conv_tf / PEAK_F32_MFMA_TFLOPS, 3)}))


if __name__ == "__main__":
    main()
