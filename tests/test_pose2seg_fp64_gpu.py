"""Pose2Seg's kernels on the MI355X against the independent fp64 restatement (tests/pose2seg_fp64.py), through their op entries.

The bit-exact tests of test_pose2seg_gpu.py compare the kernels with tests/pose2seg_ref.py, which follows the kernels' operation order;
these compare them with formulas restated in fp64, so a misconception the two share fails here.  Tolerances are derived in the docstring
of pose2seg_fp64.py, from these inputs:
  * the fp32 rounding of every warp matrix and of s = (g0 x + g1 y) + g2:  ds <= 4u (|g0 x| + |g1 y| + |g2|) + 2u |s|, zero where every
    entry, product and sum is an fp32 number;
  * the largest difference D between neighbouring taps around a sample: the value moves by at most D (|dsx| + |dsy|);
  * the bilinear mix's own roundings: 12u max|tap| (zero for integer taps at positions with 7-bit fractions);
  * a few correctly rounded fp32 operations after that (u relative each): normalisation, softmax (two exps, a sum, a divide), the
    heatmap exponent (20u relative), the limb unit vector (8u), the band distance |perp| (16u (|x - ax| + |y - ay|) + 4u);
  * the fit: normal equations solved in fp64, relative error 64 cond(S) 2^-53 in H, then rounded to fp32.
Continuous outputs (letterbox without rounding, m3 / G / Mmask / kalign, aligned features, heatmaps, limb vectors) must lie within those
bounds.  Thresholded outputs (the u8 level, the > 0.5 mask and its tight box, the limb band and its rint window, the heatmap cut at 4.6052,
the template argmin) must match exactly except where the fp64 value lies within its bound of the threshold; that ambiguous set is
asserted to stay under 0.5 % of the elements.
"""
import numpy as np
import pytest

import pose2seg_fp64 as f64
import pose2seg_run as run
from isegmi.weights import pose_templates

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("swap_rb,round_u8", [(0, 1), (1, 0), (1, 1)])
def test_letterbox_kernel_within_fp64_bounds(ffi, swap_rb, round_u8):
    rng = np.random.default_rng(100 + swap_rb)
    imgs = [f64.smooth_image(rng, *hw) for hw in ((300, 200), (97, 131), (640, 480), (2, 700), (1, 1))]
    got = run.letterbox(ffi, imgs, swap_rb, round_u8, f64.MEAN, f64.STD)
    amb = f64.Ambiguity()
    for n, im in enumerate(imgs):
        f64.check_letterbox(got[n], im, swap_rb, round_u8, amb)
    if round_u8:
        amb.check()


@pytest.mark.parametrize("align_corners,T", [(0, 3), (1, 3), (0, 1), (1, 64)])
def test_fit_kernel_within_fp64_bounds(ffi, align_corners, T):
    rng = np.random.default_rng(110 + T + align_corners)
    hws = [(480, 640), (300, 200)]
    k = np.concatenate([f64.edge_persons(rng, *hws[0]), f64.persons(rng, 8, *hws[1], invisible=0.3)])
    roi_img = np.array([0] * (len(k) - 8) + [1] * 8, np.int32)
    tp = pose_templates() if T == 3 else f64.random_templates(rng, T)
    m3, G, mm, kal, fit = run.fit(ffi, k, roi_img, hws, tp, align_corners)
    decided, ts = 0, []
    for r in range(len(k)):
        want = f64.fit(k[r], f64.m1_matrix(*hws[roi_img[r]]), tp, align_corners)
        decided += f64.check_fit(fit[r, :6], G[r], mm[r], kal[r], int(fit[r, 7]), want)
        assert np.array_equal(m3[r], fit[r, :6].astype(np.float32))
        assert np.all(np.isfinite(fit[r, :7])) and np.all(np.isfinite(G[r])) and np.all(np.isfinite(mm[r])), r   # non-finite keypoints too
        ts.append(int(fit[r, 7]))
    assert decided >= len(k) - 1
    assert -1 in ts and max(ts) >= 0                     # both the fallback and a template fit taken


@pytest.mark.parametrize("align_corners", [0, 1])
def test_align_kernel_within_fp64_bounds(ffi, align_corners):
    rng = np.random.default_rng(120 + align_corners)
    feat = rng.standard_normal((2, 128, 128, 256)).astype(np.float32)
    Hs = [[0.9, 0.15, -20.0, -0.1, 1.1, -15.0], [0.5, 0, 0, 0, 0.5, 0], [1.3, 0.2, -5.0, -0.1, 1.2, 90.0], [2.0, -0.3, 10.0, 0.4, 1.7, -60.0],
          [0.7, 0.0, 3.0, 0.0, 0.7, 5.0]]
    Hs = [np.vstack([np.reshape(h, (2, 3)), [0, 0, 1]]) for h in Hs]
    G32 = np.stack([f64.align_positions_matrix(H, align_corners).ravel() for H in Hs]).astype(np.float32)
    roi_img = np.arange(len(Hs)) % 2
    got = run.align_skeleton(ffi, feat, roi_img, G32, None, 256, skeleton=False)
    for r, H in enumerate(Hs):
        f64.check_align(got[r], feat[roi_img[r]], H, align_corners)


def test_skeleton_kernel_within_fp64_bounds(ffi):
    rng = np.random.default_rng(130)
    R = 8
    kal = np.zeros((R, 17, 3), np.float32)
    kal[..., :2] = rng.uniform(-10, 74, (R, 17, 2))
    kal[..., 2] = np.where(rng.uniform(size=(R, 17)) < 0.2, 0, 2)
    kal[1, 5, :2] = kal[1, 6, :2] = (20.0, 30.0)                   # zero-length limb
    kal[1, 7, :2] = (20.0, 50.0)                                   # axis-aligned limbs
    kal[1, 9, :2] = (44.0, 50.0)
    kal[2:5, :, :2] = rng.uniform(20, 44, (3, 17, 2))
    feat = np.zeros((1, 128, 128, 4), np.float32)
    got = run.align_skeleton(ffi, feat, np.zeros(R, np.int32), np.zeros((R, 6), np.float32), kal, 68)
    amb = f64.Ambiguity()
    for r in range(R):
        f64.check_skeleton(got[r, ..., 4:], kal[r], amb)
    amb.check()
    assert got[..., 4 + 17:4 + 55].any() and got[..., 4:4 + 17].max() > 0.9     # limb pixels and heatmap peaks present


def test_masks_kernel_within_fp64_bounds(ffi):
    rng = np.random.default_rng(140)
    hw = np.array([[50, 70], [333, 500], [90, 40]], np.int32)
    counts = np.array([2, 3, 1], np.int32)
    R, K = int(counts.sum()), 4
    logits = (np.cumsum(np.cumsum(rng.standard_normal((R, 64, 64, 2)), 1), 2) * 0.05).astype(np.float32)   # smooth logits
    logits[R - 1] = 0.75                                          # p = 0.5 exactly everywhere: an empty mask
    mm = np.zeros((R, 6), np.float32)
    owner = np.repeat(np.arange(3), counts)
    for r in range(R):
        h, w = hw[owner[r]]
        s = 64.0 / max(h, w) * rng.uniform(0.8, 2.0)
        mm[r] = (s, rng.uniform(-0.1, 0.1), rng.uniform(-10, 20), rng.uniform(-0.1, 0.1), s, rng.uniform(-10, 20))
    M, B, S, L, cnt = run.masks(ffi, logits, mm, counts, hw, K)
    amb, fg, r = f64.Ambiguity(), [], 0
    for n in range(3):
        h, w = hw[n]
        for k in range(K):
            if k < counts[n]:
                f64.check_mask(M[n, k, :h, :w], B[n, k], logits[r], mm[r], h, w, amb)
                fg.append(M[n, k, :h, :w].mean())
                r += 1
            else:
                assert not M[n, k].any() and not B[n, k].any() and S[n, k] == 0
    amb.check()
    assert fg[-1] == 0 and max(fg) > 0 and max(fg) < 1 and sum(f > 0 for f in fg) >= 3
