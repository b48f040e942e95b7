#!/usr/bin/env python3
"""The grouped 3x3 convolution (isegmi_op_conv2d_grouped) at the conv2 shapes of Mask R-CNN X-101-32x8d, 800 x 1344 canvas, bs = 2, against the
only alternative the library had before it: isegmi_op_conv2d on the block-diagonal dense expansion of the same weights (32 x the FLOPs).  Both ops run on the
same box in the same process, ALTERNATELY, `--repeats` rounds of `--reps` back-to-back launches each between two device synchronisations (host clock; a
round lasts tens of milliseconds).  Reported per shape: the median time of each, (input + output + weight bytes) / time of the grouped op next to
isegmi_box_calibrate's copy rate from the same run, and whether the two results agree bit for bit (finite inputs: the dense op only adds x * 0 products).
With --models: images/s of the X-101-32x8d and the R-101 fp32 Mask R-CNN engines, forward only on a resident batch, alternated the same way.

    python tools/grouped_conv_bench.py [--reps 50] [--repeats 5] [--models] [--out profiles/grouped_conv_bench.json]
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

N = 2
GROUPS = 32
# (stage, H, W, C, stride): conv2's INPUT.  Stride 1: the later blocks of a stage; stride 2 (STRIDE_IN_1X1 False): the stage-entry blocks of res3..res5
SHAPES = [("res2", 200, 336, 256, 1), ("res3", 100, 168, 512, 1), ("res4", 50, 84, 1024, 1), ("res5", 25, 42, 2048, 1),
          ("res3 entry", 200, 336, 512, 2), ("res4 entry", 100, 168, 1024, 2), ("res5 entry", 50, 84, 2048, 2)]


def expand(w, groups):
    C, R, S, cg = w.shape
    d = np.zeros((C, R, S, C), np.float32)
    for g in range(groups):
        d[g * cg:(g + 1) * cg, :, :, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return d


def window(ffi, launch, reps):
    ffi.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        launch()
    ffi.sync()
    return (time.perf_counter() - t0) / reps


def bench_shape(ffi, stage, H, W, C, stride, reps, repeats):
    rng = np.random.default_rng(C * 10 + stride)
    cg = C // GROUPS
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((C, 3, 3, cg)) * np.sqrt(2.0 / (9 * cg))).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32); shift = (rng.standard_normal(C) * 0.1).astype(np.float32)
    d = ffi.make_conv_desc(N, H, W, C, C, 3, 3, stride, 1, 1)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dx = ffi.DeviceBuffer.from_numpy(x)
    dwg = ffi.DeviceBuffer.from_numpy(ffi.pack_conv_weights_grouped(d, GROUPS, w))
    dwd = ffi.DeviceBuffer.from_numpy(ffi.pack_conv_weights(d, expand(w, GROUPS)))
    ds, dh = ffi.DeviceBuffer.from_numpy(scale), ffi.DeviceBuffer.from_numpy(shift)
    og, od = ffi.DeviceBuffer((N, Ho, Wo, C)).poison(), ffi.DeviceBuffer((N, Ho, Wo, C)).poison()
    grouped = lambda: ffi.op_conv2d_grouped(d, GROUPS, dx, dwg, ds, dh, None, og)
    dense = lambda: ffi.op_conv2d(d, dx, dwd, ds, dh, None, od)
    for f in (grouped, dense):   # warm-up: code objects, the LDS limit, clocks
        window(ffi, f, max(3, reps // 5))
    tg, td = [], []
    for _ in range(repeats):
        tg.append(window(ffi, grouped, reps)); td.append(window(ffi, dense, reps))
    a, b = og.numpy(), od.numpy()
    nbytes = 4 * (x.size + a.size + w.size)
    mg, md = float(np.median(tg)), float(np.median(td))
    out = {"stage": stage, "input": [N, H, W, C], "stride": stride, "channels_per_group": cg, "grouped_us": [round(t * 1e6, 1) for t in tg],
           "dense_block_diagonal_us": [round(t * 1e6, 1) for t in td], "grouped_median_us": round(mg * 1e6, 1), "dense_median_us": round(md * 1e6, 1),
           "grouped_faster": bool(max(tg) < min(td)), "speedup": round(md / mg, 2), "algorithmic_bytes": int(nbytes),
           "grouped_gbs": round(nbytes / mg / 1e9, 1), "grouped_gflops": round(2.0 * a.size * 9 * cg / mg / 1e9, 1),
           "results_bit_identical": bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))), "finite": bool(np.isfinite(a).all())}
    for buf in (dx, dwg, dwd, ds, dh, og, od):
        buf.free()
    return out


def bench_models(steps, warmup, repeats):
    from fasterrcnn_bench import timed
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import random_maskrcnn_state_dict
    H, W = 800, 1344
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(N)]
    cfgs = {"R-101-FPN fp32": MaskRCNNConfig(depth=101, CONV_BODY="R-101-FPN"),
            "X-101-32x8d-FPN fp32": MaskRCNNConfig(depth=101, CONV_BODY="R-101-FPN", NUM_GROUPS=32, WIDTH_PER_GROUP=8, STRIDE_IN_1X1=False)}
    nets, out = {}, {}
    for name, cfg in cfgs.items():
        net = MaskRCNN(random_maskrcnn_state_dict(cfg, 1234), H, W, cfg=cfg, max_batch=N)
        net.reserve(); net.upload_u8(imgs)
        nets[name] = net
        out[name] = {"images_per_s": [], "p50_step_ms": []}
    for _ in range(repeats):
        for name, net in nets.items():
            ips, p50 = timed(net, N, steps, warmup)
            out[name]["images_per_s"].append(round(ips, 2)); out[name]["p50_step_ms"].append(None if p50 is None else round(p50, 3))
    for net in nets.values():
        net.close()
    return {"canvas": [H, W], "batch": N, "steps": steps, "note": "forward only on a resident batch, seeded random weights", "engines": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_conv_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    res = {"box": _ffi.box_calibrate(), "reps": a.reps, "repeats": a.repeats, "groups": GROUPS,
           "shapes": [bench_shape(_ffi, *s, a.reps, a.repeats) for s in SHAPES]}
    copy = res["box"]["hbm_copy_gbs"]
    for s in res["shapes"]:
        s["fraction_of_copy_rate"] = round(s["grouped_gbs"] / copy, 3)
    res["grouped_faster_at_every_shape"] = all(s["grouped_faster"] for s in res["shapes"])
    if a.models:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res["models"] = bench_models(a.steps, 2, 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if res["grouped_faster_at_every_shape"] else 1


if __name__ == "__main__":
    sys.exit(main())
