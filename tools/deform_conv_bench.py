#!/usr/bin/env python3
"""The fused deformable convolution (isegmi_op_deform_conv2d) against the unfused form it replaces (isegmi_op_deform_im2col, then
isegmi_op_conv2d as a 1x1 over 9 C channels; the offset convolution belongs to both forms and is timed in neither) at the conv2 shapes of the dcn/ R-CNN
models -- 800 x 1344 canvas, bs = 2 and bs = 1 -- and of YOLACT++ at 550 x 550.  Both forms run in one process, ALTERNATELY: 5 warm-up windows each, then
`--rounds` rounds of one window per form; a window is `--reps` back-to-back launches between two HIP events on the null stream.  Reported per shape: the
median of each form, the column bytes the fused form does not move (written once, read once), TFLOP/s of the fused form against isegmi_box_calibrate's fp32
MFMA rate (read before and after, same process), and whether the two results agree bit for bit.  Seeded random weights; offsets at the synthetic +-1 pixel
scale of the seeded state dicts (YOLACT_DCN_OFFSET_STD), mask logits around 0.
With --models: the mdconv Mask R-CNN R-50-FPN step with dcn_fused 0 and 1 (one engine, the parameter switched) next to the plain R-50-FPN step, bs = 2 and
bs = 1, forward only on a resident batch, alternated the same way.

    python tools/deform_conv_bench.py [--reps 10] [--rounds 20] [--models] [--out profiles/deform_conv_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "instancesegmentation-jittor_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

WARMUP = 5
# (name, N, H, W, C, stride): conv2's INPUT.  R-CNN (STRIDE_IN_1X1 True): the stride sits on conv1, every conv2 is stride 1.  YOLACT++ (torchvision form): the
# stage-entry blocks of res3..res5 carry the stride on the deformable 3x3.
RCNN = [("res3", 100, 168, 128), ("res4", 50, 84, 256), ("res5", 25, 42, 512)]
SHAPES = [("rcnn %s bs%d" % (s, n), n, h, w, c, 1) for n in (2, 1) for s, h, w, c in RCNN] + \
         [("yolact++ res3 entry", 1, 138, 138, 128, 2), ("yolact++ res3", 1, 69, 69, 128, 1), ("yolact++ res4 entry", 1, 69, 69, 256, 2),
          ("yolact++ res4", 1, 35, 35, 256, 1), ("yolact++ res5 entry", 1, 35, 35, 512, 2), ("yolact++ res5", 1, 18, 18, 512, 1)]


def bench_shape(ffi, ev, name, N, H, W, C, stride, reps, rounds, f32_tflops):
    from isegmi.weights import YOLACT_DCN_OFFSET_STD
    rng = np.random.default_rng([C, H, W, N, stride])
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = np.maximum(rng.standard_normal((N, H, W, C)), 0).astype(np.float32)   # post-ReLU activations
    om = (rng.standard_normal((N, Ho, Wo, 27)) * YOLACT_DCN_OFFSET_STD).astype(np.float32)
    w = (rng.standard_normal((C, 1, 1, 9 * C)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32); shift = (rng.standard_normal(C) * 0.1).astype(np.float32)
    d = ffi.make_conv_desc(N, Ho, Wo, 9 * C, C, 1, 1, 1, 0, 1)
    dx, dom = ffi.DeviceBuffer.from_numpy(x), ffi.DeviceBuffer.from_numpy(om)
    dw = ffi.DeviceBuffer.from_numpy(ffi.pack_conv_weights(d, w))   # ONE packed image serves both forms
    ds, dh = ffi.DeviceBuffer.from_numpy(scale), ffi.DeviceBuffer.from_numpy(shift)
    col = ffi.DeviceBuffer((N, Ho, Wo, 9 * C))
    of, ou = ffi.DeviceBuffer((N, Ho, Wo, C)).poison(), ffi.DeviceBuffer((N, Ho, Wo, C)).poison()
    L = ffi.lib()

    def fused():
        ffi.check(L.isegmi_op_deform_conv2d(dx.ptr, N, H, W, C, dom.ptr, 27, 1, stride, dw.ptr, C, ds.ptr, dh.ptr, None, 1, of.ptr, None))

    def unfused():
        ffi.check(L.isegmi_op_deform_im2col(dx.ptr, N, H, W, C, dom.ptr, 3, 3, stride, 1, 1, col.ptr, None))
        ffi.op_conv2d(d, col, dw, ds, dh, None, ou)

    def im2col_only():
        ffi.check(L.isegmi_op_deform_im2col(dx.ptr, N, H, W, C, dom.ptr, 3, 3, stride, 1, 1, col.ptr, None))
    for _ in range(WARMUP):
        ev.time_us(fused, reps); ev.time_us(unfused, reps)
    tf, tu, ti = [], [], []
    for _ in range(rounds):
        tf.append(ev.time_us(fused, reps)); tu.append(ev.time_us(unfused, reps)); ti.append(ev.time_us(im2col_only, reps))
    a, b = of.numpy(), ou.numpy()
    mf, mu, mi = float(np.median(tf)), float(np.median(tu)), float(np.median(ti))
    flops = 2.0 * N * Ho * Wo * 9 * C * C
    out = {"shape": name, "input": [N, H, W, C], "stride": stride, "M": N * Ho * Wo, "K": 9 * C, "Cout": C,
           "fused_median_us": round(mf, 1), "two_launch_median_us": round(mu, 1), "im2col_alone_median_us": round(mi, 1),
           "fused_min_max_us": [round(min(tf), 1), round(max(tf), 1)], "two_launch_min_max_us": [round(min(tu), 1), round(max(tu), 1)],
           "fused_over_two_launch": round(mf / mu, 3), "fused_not_slower": bool(mf <= mu),
           "column_bytes_avoided": int(2 * 4 * N * Ho * Wo * 9 * C), "gflop": round(flops / 1e9, 2),
           "fused_tflops": round(flops / mf / 1e6, 2), "two_launch_tflops": round(flops / mu / 1e6, 2),
           "fused_fraction_of_calibrated_f32_mfma": round(flops / mf / 1e6 / f32_tflops, 3),
           "results_bit_identical": bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))), "finite": bool(np.isfinite(a).all())}
    for buf in (dx, dom, dw, ds, dh, col, of, ou):
        buf.free()
    return out


def bench_models(steps, warmup, repeats):
    from fasterrcnn_bench import timed
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.weights import random_maskrcnn_state_dict
    H, W, N = 800, 1344, 2
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(N)]
    cfgs = {"plain": MaskRCNNConfig(depth=50, CONV_BODY="R-50-FPN"),
            "mdconv": MaskRCNNConfig(depth=50, CONV_BODY="R-50-FPN", STAGE_WITH_DCN=(False, True, True, True), WITH_MODULATED_DCN=True)}
    nets = {}
    for name, cfg in cfgs.items():
        net = MaskRCNN(random_maskrcnn_state_dict(cfg, 1234), H, W, cfg=cfg, max_batch=N)
        net.reserve(); net.upload_u8(imgs)
        nets[name] = net
    runs = (("R-50-FPN plain", "plain", None), ("R-50-FPN mdconv dcn_fused=0", "mdconv", 0.0), ("R-50-FPN mdconv dcn_fused=1", "mdconv", 1.0))
    out = {}
    for bs in (2, 1):
        res = {label: {"images_per_s": [], "p50_step_ms": []} for label, _, _ in runs}
        for _ in range(repeats):
            for label, which, fused in runs:
                if fused is not None:
                    nets[which].set_param("dcn_fused", fused)
                ips, p50 = timed(nets[which], bs, steps, warmup)
                res[label]["images_per_s"].append(round(ips, 2)); res[label]["p50_step_ms"].append(None if p50 is None else round(p50, 3))
        for r in res.values():
            r["median_images_per_s"] = float(np.median(r["images_per_s"]))
        out["bs%d" % bs] = res
    for net in nets.values():
        net.close()
    return {"canvas": [H, W], "steps": steps, "note": "fp32, forward only on a resident batch, seeded random weights", "engines": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_conv_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    from yolov3_bench import Events
    _ffi.set_device(0)
    box = _ffi.box_calibrate()
    ev = Events()
    res = {"box_before": box, "reps": a.reps, "rounds": a.rounds, "warmup_windows": WARMUP,
           "shapes": [bench_shape(_ffi, ev, *s, a.reps, a.rounds, box["mfma_f32_tflops"]) for s in SHAPES]}
    bs2 = [s for s in res["shapes"] if s["shape"].startswith("rcnn") and s["input"][0] == 2]
    res["rcnn_bs2_fused_not_slower"] = {s["shape"]: s["fused_not_slower"] for s in bs2}
    # the rule of DESIGN.md 19: 1 if the fused median is not above the two-launch one at each bs = 2 shape; otherwise per stage, a losing stage keeps 0
    res["rcnn_default_dcn_fused"] = 1 if all(s["fused_not_slower"] for s in bs2) else {s["shape"].split()[1]: int(s["fused_not_slower"]) for s in bs2}
    res["all_bit_identical"] = all(s["results_bit_identical"] for s in res["shapes"])
    if a.models:
        res["models"] = bench_models(a.steps, 2, 3)
    res["box_after"] = _ffi.box_calibrate()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if res["all_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
