"""GroupNorm kernels and the GroupNorm Mask R-CNN, measured.

    python tools/groupnorm_bench.py [--out profiles/groupnorm_bench.txt] [--iters 50] [--steps 20] [--no-model]

Per GroupNorm launch shape of R50-FPN at 800 x 1344, bs = 2 (the list below): algorithmic bytes, microseconds and GB/s next to the float4 copy
rate isegmi_box_calibrate measures in the same process, and their ratio.  Algorithmic bytes: a slab launch (H * W <= 196) reads x and writes y once
(2 x 4 B per element); a plane launch reads x in the statistics pass and again in the apply pass and writes y (3 x 4 B per element) -- against a copy
that reads and writes once, a plane launch at the copy's rate would show 1.0 here and cannot move fewer bytes.  Then the whole forward: the GroupNorm
model's ms per step next to the FrozenBN model's on the same box.  Times are wall clock over `iters` back-to-back launches between two device syncs.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "instancesegmentation-jittor_amd")]

# (label, N, H, W, C, residual, relu): the distinct GroupNorm launches of one R50-FPN forward at 800 x 1344, bs = 2, 32 groups
SHAPES = [
    ("stem", 2, 400, 672, 64, False, True),
    ("res2 conv1/conv2", 2, 200, 336, 64, False, True),
    ("res2 conv3 + identity", 2, 200, 336, 256, True, True),
    ("res3 conv3 + identity", 2, 100, 168, 512, True, True),
    ("res4 conv3 + identity", 2, 50, 84, 1024, True, True),
    ("res5 conv3 + identity", 2, 25, 42, 2048, True, True),
    ("FPN P2 output", 2, 200, 336, 256, False, False),
    ("box head xconv, 1000 RoIs/image", 2000, 7, 7, 256, False, True),
    ("mask head fcn, 100 RoIs/image", 200, 14, 14, 256, False, True),
]


def time_kernel(ffi, N, H, W, C, residual, relu, iters):
    rng = np.random.default_rng(0)
    dx = ffi.DeviceBuffer.from_numpy(rng.standard_normal((N, H, W, C), np.float32))
    do = ffi.DeviceBuffer((N, H, W, C))
    dr = ffi.DeviceBuffer.from_numpy(rng.standard_normal((N, H, W, C), np.float32)) if residual else None
    dg = ffi.DeviceBuffer.from_numpy(np.ones(C, np.float32)); db = ffi.DeviceBuffer.from_numpy(np.zeros(C, np.float32))
    ws = ffi.group_norm_device(dx, N, H, W, C, 32, dg, db, 1e-5, dr, relu, do)
    for _ in range(3):
        ffi.group_norm_device(dx, N, H, W, C, 32, dg, db, 1e-5, dr, relu, do, ws)
    ffi.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        ffi.group_norm_device(dx, N, H, W, C, 32, dg, db, 1e-5, dr, relu, do, ws)
    ffi.sync()
    return (time.perf_counter() - t0) / iters * 1e6


def time_model(gn, steps, warmup=5):
    import dataclasses
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import maskrcnn_state_dict
    cfg = MaskRCNNConfig()
    if gn:
        cfg = dataclasses.replace(cfg, USE_GN=True, STRIDE_IN_1X1=False, BOX_HEAD="FPNXconv1fcFeatureExtractor")
    net = MaskRCNN(maskrcnn_state_dict(1234, gn=gn), 800, 1344, cfg=cfg, max_batch=2)
    rng = np.random.default_rng(1)
    x = (rng.uniform(0, 255, (2, 800, 1344, 3)) - 115.0).astype(np.float32)
    net.upload(x, np.array([[800, 1344], [800, 1344]], np.int32))
    for _ in range(warmup):
        net.forward_device(2)
    net.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.forward_device(2)
    net.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    det = int(net.fetch("det.count", 2).sum())
    net.close()
    return ms, det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupnorm_bench.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    from isegmi import _ffi as ffi
    ffi.set_device(0)
    box = ffi.box_calibrate()
    copy = box["hbm_copy_gbs"]
    lines = ["GroupNorm kernels, R50-FPN 800x1344 bs=2 launch shapes, 32 groups (tools/groupnorm_bench.py)",
             "box: %s" % box,
             "%-34s %-20s %-6s %10s %9s %9s %8s" % ("layer", "N x H x W x C", "regime", "bytes", "us", "GB/s", "/ copy")]
    for label, N, H, W, C, res, relu in SHAPES:
        slab = H * W <= 196
        nbytes = N * H * W * C * 4 * ((2 if slab else 3) + (1 if res else 0))
        us = time_kernel(ffi, N, H, W, C, res, relu, a.iters)
        gbs = nbytes / us / 1e3
        lines.append("%-34s %-20s %-6s %10d %9.1f %9.1f %8.2f" % (label, "%dx%dx%dx%d" % (N, H, W, C), "slab" if slab else "plane", nbytes, us, gbs, gbs / copy))
    if not a.no_model:
        bn_ms, bn_det = time_model(False, a.steps)
        gn_ms, gn_det = time_model(True, a.steps)
        lines.append("forward, 800x1344 bs=2 fp32, ms per step: FrozenBN %.2f (%d detections)   GroupNorm %.2f (%d detections)   ratio %.2f" % (
            bn_ms, bn_det, gn_ms, gn_det, gn_ms / bn_ms))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
