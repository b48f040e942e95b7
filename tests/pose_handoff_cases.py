"""Hand-built inputs of the Keypoint R-CNN -> Pose2Seg hand-off, shared by the CPU tests (which prove that each one tells the
right rule from a wrong one) and the GPU tests (which run the kernel on them).  Every case is the keyword set of pose_handoff_ref.handoff."""
import numpy as np

RATIOS = (1.37, 0.81)


def _fill(rng, N, cap):
    """keypoints, logits and ratios for N x cap slots: nothing is zero or one, so a missed scale or a missed copy shows"""
    kpt = rng.uniform(3, 400, (N, cap, 17, 3)).astype(np.float32)
    kpt[..., 2] = 1
    kscore = rng.uniform(-4, 9, (N, cap, 17)).astype(np.float32)
    ratios = np.array([[RATIOS[0] + 0.11 * n, RATIOS[1] - 0.07 * n] for n in range(N)], np.float32)
    return kpt, kscore, ratios


def _case(score, count, seed, person_thresh=0.5, kp_thresh=2.0, K=4):
    score = np.asarray(score, np.float32)
    kpt, kscore, ratios = _fill(np.random.default_rng(seed), *score.shape)
    return dict(score=score, count=np.asarray(count, np.int32), kpt=kpt, kscore=kscore, ratios=ratios, person_thresh=person_thresh, kp_thresh=kp_thresh, K=K)


def _poison_dead_slots(c):
    """stale garbage behind every image's count, non-finite values included"""
    for n, cn in enumerate(c["count"]):
        dead = c["score"].shape[1] - int(cn)
        c["score"][n, cn:] = np.resize(np.float32([np.inf, np.nan, 0.99, -np.inf, 3e38, 0.75]), dead)
        c["kpt"][n, cn:] = np.nan
        c["kscore"][n, cn:] = np.inf
    return c


def single_case():
    """N = 1, cap = 1"""
    return _case([[0.8]], [1], 1, K=1)


def threshold_case():
    """scores one ulp above, at and one ulp below the person threshold; of the person that passes, logits at, above and below the keypoint threshold"""
    t = np.float32(0.5)
    c = _case([[np.nextafter(t, np.float32(1)), t, np.nextafter(t, np.float32(0)), 0.9]], [3], 2, person_thresh=0.5, kp_thresh=2.0, K=4)
    k = np.float32(2.0)
    c["kscore"][0, 0, :3] = [k, np.nextafter(k, np.float32(3)), np.nextafter(k, np.float32(0))]
    return _poison_dead_slots(c)


def ties_case(K):
    """blocks of equal scores: K = 3 cuts inside the 0.8 block, K = 4 ends on it, K = 6 cuts inside the 0.7 block"""
    return _poison_dead_slots(_case([[0.9, 0.7, 0.7, 0.8, 0.7, 0.6, 0.8, 0.7, 0.3, 0.9, 0.0, 0.0]], [10], 3, K=K))


def ascending_case():
    """100 distinct scores in ascending slot order, more candidates than K"""
    return _case([np.linspace(0.3, 0.99, 100)], [100], 4, K=4)


def batch_case(K):
    """N = 3, cap = 100, counts (0, 5, 100); image 1 has exactly four candidates (K = 1: more, 4: as many, 128: fewer), image 2 about fifty with ties"""
    rng = np.random.default_rng(5)
    score = np.round(rng.uniform(0, 1, (3, 100)), 2).astype(np.float32)
    score[1, :5] = [0.6, 0.2, 0.9, 0.6, 0.7]
    return _poison_dead_slots(_case(score, [0, 5, 100], 6, K=K))


def empty_case():
    """no image has a detection: R = 0"""
    return _poison_dead_slots(_case(np.full((2, 8), 0.9), [0, 0], 7, K=4))


def all_cut_case():
    """image 1 has detections, none above the threshold (one exactly at it)"""
    return _poison_dead_slots(_case([[0.9, 0.1, 0.7, 0, 0, 0], [0.5, 0.2, 0.49, 0.3, 0, 0], [0.2, 0.8, 0, 0, 0, 0]], [3, 4, 2], 8, K=4))


def all_cases():
    out = {"single": single_case(), "threshold": threshold_case(), "ascending": ascending_case(), "empty": empty_case(), "all_cut": all_cut_case()}
    out.update({"ties_K%d" % K: ties_case(K) for K in (3, 4, 6)})
    out.update({"batch_K%d" % K: batch_case(K) for K in (1, 4, 128)})
    return out
