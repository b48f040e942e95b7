#!/usr/bin/env python3
"""Test-time box augmentation against the plain forwards it is made of, in one process: the shipped yaml
(configs/e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml: ten views) on 800 x 1333 images, seeded random weights, bs = 1 and 2.

Per batch size, `--repeats` times each and ALTERNATELY: the wall time of MaskRCNN.detect_aug (host resizes, one upload, ten views, merge, the fetch of the
results) next to the SUM of plain passes over the same ten canvases -- per view the same host resize (and a host-side mirror image), upload_u8,
forward_device, sync and the fetch of det.*.  Then, under op_timing, the device time of the two stages the feature adds -- the per-view candidate stage and
the merge -- next to the device time of a plain forward of the identity view (HIP events around it).

    python tools/bbox_aug_bench.py [--repeats 3] [--out profiles/bbox_aug_bench.json]
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

H, W = 800, 1333
STAGES = ("bbox_aug_candidates", "bbox_aug_merge")


def op_stats(net):
    from isegmi import _ffi
    cap = 64
    names = C.create_string_buffer(16384)
    us, by, ln, cnt = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int()
    _ffi.check(_ffi.lib().isegmi_engine_op_stats(net._h, names, 16384, us, by, ln, cap, C.byref(cnt)))
    labels = names.value.decode().split("\n") if cnt.value else []
    return {labels[i]: (float(us[i]), int(ln[i])) for i in range(cnt.value)}


def plain_views(net, mc, aug, imgs):
    """The ten views as ten plain passes.  -> seconds"""
    from isegmi.transforms import maskrcnn_resize_u8
    t0 = time.perf_counter()
    for mn, mx, flip in [(mc.MIN_SIZE_TEST, mc.MAX_SIZE_TEST, aug.H_FLIP)] + [(s, aug.MAX_SIZE, aug.SCALE_H_FLIP) for s in aug.SCALES]:
        rs = [maskrcnn_resize_u8(im, mn, mx) for im in imgs]
        for hflip in ((False, True) if flip else (False,)):
            n = net.upload_u8([np.ascontiguousarray(r[:, ::-1]) for r in rs] if hflip else rs)
            net.forward_device(n)
            net.sync()
            for k in ("det.count", "det.box", "det.score", "det.label"):
                net.fetch(k, n)
    return time.perf_counter() - t0


def run(bs, repeats):
    from isegmi.config import cfg, to_bbox_aug_config
    from isegmi.maskrcnn import MaskRCNN, bbox_aug_engine_side, bbox_aug_views
    from isegmi.transforms import maskrcnn_resize_u8
    from isegmi.weights import random_maskrcnn_state_dict
    c = cfg.clone()
    c.merge_from_file(os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x_bbox_aug.yaml"))
    mc, aug = to_bbox_aug_config(c)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), np.uint8) for _ in range(bs)]
    side = bbox_aug_engine_side(mc, aug)
    net = MaskRCNN(random_maskrcnn_state_dict(mc, 1234), side, side, cfg=mc, max_batch=bs)
    out = {"batch": bs, "image": [H, W], "engine_canvas": [side, side], "views": [list(v) for v in bbox_aug_views((H, W), mc, aug)],
           "detect_aug_ms": [], "plain_sum_ms": []}
    try:
        net.reserve()
        from isegmi.maskrcnn import BBoxAugOverflow
        for thr in (mc.ROI_SCORE_THRESH, 0.1, 0.2, 0.4):   # random weights score near-uniformly: the threshold under which ten views fit the pool
            net.set_param("roi_score_thresh", float(thr))
            try:
                net.detect_aug(imgs, aug)                  # (also the warm-up: every buffer at its final size)
                break
            except BBoxAugOverflow as e:
                out.setdefault("overflowed_at", []).append([float(thr), str(e)])
        out["roi_score_thresh"] = float(thr)
        plain_views(net, mc, aug, imgs)
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = net.detect_aug(imgs, aug)
            out["detect_aug_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            out["plain_sum_ms"].append(round(plain_views(net, mc, aug, imgs) * 1e3, 2))
        out["detections"] = [len(r) for r in res]
        out["pool_total"] = net.fetch("aug.pool_total", bs).tolist()
        # device time of the added stages (ten candidate stages + one merge per pass) and of one plain forward of the identity view
        net.set_param("op_timing", 1.0)
        op_stats(net)
        for _ in range(repeats):
            net.detect_aug(imgs, aug)
        st = op_stats(net)
        net.set_param("op_timing", 0.0)
        for key in STAGES:
            hit = [(us, ln) for label, (us, ln) in st.items() if label.startswith(key)]
            us, ln = (sum(h[0] for h in hit), sum(h[1] for h in hit)) if hit else (0.0, 0)
            out[key + "_us_per_call"] = round(us / max(ln, 1), 2)
            out[key + "_calls_per_pass"] = ln // repeats
        n = net.upload_u8([maskrcnn_resize_u8(im, mc.MIN_SIZE_TEST, mc.MAX_SIZE_TEST) for im in imgs])
        net.forward_device(n); net.sync(); net.step_times()
        net.mark_step()
        for _ in range(5):
            net.forward_device(n)
            net.mark_step()
        net.sync()
        ms = sorted(net.step_times())
        out["plain_forward_identity_view_ms"] = round(ms[len(ms) // 2], 3)
    finally:
        net.close()
    a, p = float(np.median(out["detect_aug_ms"])), float(np.median(out["plain_sum_ms"]))
    out["detect_aug_over_plain_sum"] = round(a / p, 4)
    out["added_stages_share_of_identity_forward"] = round((out["bbox_aug_candidates_us_per_call"] + out["bbox_aug_merge_us_per_call"] / max(len(out["views"]), 1))
                                                          / (out["plain_forward_identity_view_ms"] * 1e3), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbox_aug_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    res = {"weights": "random (seed 1234)", "repeats": a.repeats,
           "note": "wall times include the host's PIL resizes on both sides; added_stages_share = (one candidate stage + a tenth of the merge) / one plain forward of the identity view",
           "runs": [run(bs, a.repeats) for bs in (1, 2)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
