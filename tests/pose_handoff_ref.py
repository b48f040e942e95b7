"""numpy restatement of the Keypoint R-CNN -> Pose2Seg hand-off (csrc/pose_handoff.hip), in fp32.

    handoff(score [N, cap], count [N], kpt [N, cap, 17, 3], kscore [N, cap, 17], ratios [N, 2] = (ratio_w, ratio_h), person_thresh, kp_thresh, K)
        -> kpts_out [R, 17, 3], score_out [N, K], src_slot [N, K] int32, count_out [N] int32

A slot j < count[n] is a candidate when score > person_thresh (strict); the min(#candidates, K) best are kept, by score descending, equal scores by slot
ascending; the input need not be sorted.  Keypoint k of a kept person is (x * ratio_w, y * ratio_h, v), one fp32 multiplication each, v = 2 where
kscore > kp_thresh (strict), else 0.  Persons are packed image by image.  Slots at or beyond count[n] are never looked at."""
import numpy as np


def select(score, count, person_thresh, K):
    """-> the detection slots of the kept persons of one image, best first"""
    s = np.asarray(score, np.float32)[:int(count)]
    cand = np.flatnonzero(s > np.float32(person_thresh))
    order = cand[np.argsort(-s[cand], kind="stable")]      # descending; a stable sort leaves equal scores in slot order
    return order[:K]


def handoff(score, count, kpt, kscore, ratios, person_thresh, kp_thresh, K):
    score, kpt, kscore = (np.asarray(a, np.float32) for a in (score, kpt, kscore))
    ratios = np.asarray(ratios, np.float32).reshape(-1, 2)
    N = score.shape[0]
    assert kpt.shape[2:] == (17, 3) and kscore.shape == kpt.shape[:3]
    score_out = np.zeros((N, K), np.float32)
    src_slot = np.full((N, K), -1, np.int32)
    count_out = np.zeros(N, np.int32)
    rows = []
    for n in range(N):
        sel = select(score[n], count[n], person_thresh, K)
        c = len(sel)
        count_out[n] = c
        score_out[n, :c] = score[n, sel]
        src_slot[n, :c] = sel
        k = np.empty((c, 17, 3), np.float32)
        k[:, :, 0] = kpt[n, sel, :, 0] * ratios[n, 0]
        k[:, :, 1] = kpt[n, sel, :, 1] * ratios[n, 1]
        k[:, :, 2] = np.where(kscore[n, sel] > np.float32(kp_thresh), np.float32(2), np.float32(0))
        rows.append(k)
    return np.concatenate(rows) if rows else np.zeros((0, 17, 3), np.float32), score_out, src_slot, count_out


def split(kpts_out, count_out):
    """the packed rows as one (n_i, 17, 3) array per image"""
    off = np.concatenate([[0], np.cumsum(count_out)])
    return [kpts_out[off[i]:off[i + 1]] for i in range(len(count_out))]
