#!/usr/bin/env python3
"""Person segmentation from images alone: ms per step of isegmi.pose2seg.KeypointPose2Seg -- Keypoint R-CNN, the device hand-off,
Pose2Seg -- next to its two parts measured alone in the same process on the same images: the detector step (uint8 upload + forward) and the Pose2Seg
step fed the SAME keypoints from the host (Pose2Seg.forward).  bs images of 512 x 512 uint8, both models at the paper's widths with seeded synthetic
weights; the person threshold is the median of the detector's own scores on these images, so about half of the detections become persons (at most
--max-instances per image).  Steps are enqueued back to back and each loop is synchronised at its end; the three loops are interleaved over --rounds
so that a drift of the box hits all three alike.  The expectation to check: pipeline <= detector + pose2seg (the count download hides behind
Pose2Seg's backbone).  The two parts run free -- the host is steps ahead of the GPU --, the pipeline's host waits once per step for the counts, so what
the host does before it can enqueue the next detector forward (resize, staging: `host_prep_ms_per_step`, measured apart) is exposed there.

    python tools/person_seg_bench.py [--batch 8] [--steps 20] [--warmup 3] [--rounds 3] [--max-instances 8] [--out profiles/person_seg_bench.txt]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512, help="side of the square originals; the detector runs at this size too")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-instances", dest="max_instances", type=int, default=8)
    ap.add_argument("--score-thresh", dest="score_thresh", type=float, default=0.012, help="the detector's ROI_HEADS.SCORE_THRESH (seeded weights score low)")
    ap.add_argument("--out", default=None, help="also append the result line to this file")
    a = ap.parse_args()
    from isegmi import _ffi
    from isegmi.maskrcnn import MaskRCNN, MaskRCNNConfig
    from isegmi.pose2seg import KeypointPose2Seg, Pose2Seg, Pose2SegConfig
    from isegmi.weights import keypointrcnn_state_dict, pose2seg_state_dict
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (a.size, a.size, 3), np.uint8) for _ in range(a.batch)]
    cfg = dataclasses.replace(MaskRCNNConfig(), MASK_ON=False, NUM_CLASSES=2, KEYPOINT_ON=True, ROI_SCORE_THRESH=a.score_thresh, MIN_SIZE_TEST=a.size,
                              MAX_SIZE_TEST=a.size)
    side = -(-a.size // cfg.SIZE_DIVISIBILITY) * cfg.SIZE_DIVISIBILITY
    det = MaskRCNN(keypointrcnn_state_dict(1234), side, side, cfg=cfg, max_batch=a.batch)
    net = Pose2Seg(pose2seg_state_dict(1234), Pose2SegConfig(), max_batch=a.batch, max_instances=a.max_instances)
    # the thresholds from the detector's own answer: the median score, the median keypoint logit
    bls = det(imgs)
    scores = np.concatenate([b.get_field("scores") for b in bls])
    logits = np.concatenate([b.get_field("keypoint_logits").ravel() for b in bls])
    if len(scores) == 0:
        raise SystemExit("the detector found nothing on these images: lower --score-thresh")
    pipe = KeypointPose2Seg(det, net, person_threshold=float(np.median(scores)), keypoint_threshold=float(np.median(logits)))
    kps = [g[3] for g in pipe(imgs)]            # the keypoints the pipeline itself hands over, for the host-fed Pose2Seg step
    persons = [len(k) for k in kps]
    hw = [im.shape[:2] for im in imgs]
    pin = _ffi.PinnedBuffer((sum(im.size for im in imgs),), np.uint8)
    pin.array[:] = np.concatenate([im.reshape(-1) for im in imgs])

    def detector_step():
        det.upload_u8_async(pin, hw, 0)
        det.forward_device(a.batch, 0)

    def host_prep():   # what a pipeline step does on the host before it can enqueue the detector: COCODemo's resize, the images into pinned memory
        from isegmi.transforms import maskrcnn_resize_u8
        t0 = time.perf_counter()
        off = 0
        for im in imgs:
            r = maskrcnn_resize_u8(im, a.size, a.size)
            pin.array[off:off + r.size] = r.reshape(-1)
            off += r.size
        return (time.perf_counter() - t0) * 1e3
    prep = float(np.median([host_prep() for _ in range(5)]))

    legs = {"pipeline": (lambda: pipe.forward(imgs), pipe.sync), "detector": (detector_step, det.sync), "pose2seg_host_keypoints": (lambda: net.forward(imgs, kps), net.sync)}
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for name, (step, sync) in legs.items():
            for _ in range(a.warmup):
                step()
            sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            sync()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    pipe.close(); net.close(); det.close(); pin.free()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"model": "keypointrcnn_r50_fpn + pose2seg", "batch": a.batch, "image": [a.size, a.size], "detections": int(len(scores)), "persons": persons,
           "max_instances": a.max_instances, "steps": a.steps, "rounds": a.rounds,
           "ms_per_step": {k: round(v, 3) for k, v in med.items()}, "ms_per_step_rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "host_prep_ms_per_step": round(prep, 3),
           "sum_of_parts_ms": round(med["detector"] + med["pose2seg_host_keypoints"], 3),
           "pipeline_over_sum": round(med["pipeline"] / (med["detector"] + med["pose2seg_host_keypoints"]), 4),
           "images_per_s": round(a.batch / med["pipeline"] * 1e3, 2)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
