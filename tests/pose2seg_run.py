"""Pose2Seg's five op entries (isegmi_op_pose2seg_*) run once each from host arrays, for the GPU tests.  Test infrastructure only."""
import numpy as np

import pose2seg_fp64 as f64


def dev(a):
    from isegmi import _ffi
    return _ffi.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def letterbox(ffi, imgs, swap_rb, round_u8, mean, std):
    """-> [N, 512, 512, 4]"""
    from isegmi.pose2seg import letterbox_inverse, letterbox_matrix
    offs = np.cumsum([0] + [im.size for im in imgs])
    table = (ffi.P2sImage * len(imgs))()
    for n, im in enumerate(imgs):
        table[n].offset, table[n].h, table[n].w = int(offs[n]), im.shape[0], im.shape[1]
        table[n].minv[:] = letterbox_inverse(letterbox_matrix(*im.shape[:2]))
    out = ffi.DeviceBuffer((len(imgs), 512, 512, 4))
    ffi.p2s_letterbox(dev(np.concatenate([im.ravel() for im in imgs])), dev(np.frombuffer(bytes(table), np.uint8)), len(imgs), 512, mean, std,
                      swap_rb, round_u8, out)
    return out.numpy()


def m1s(hws):
    return np.array([f64.m1_matrix(h, w)[:2].ravel() for h, w in hws])


def fit(ffi, k, roi_img, hws, tp, align_corners):
    """-> m3 [R, 6], G [R, 6], mmask [R, 6] fp32, kalign [R, 17, 3], fit [R, 8] fp64 (m3, err, t)"""
    R = len(k)
    outs = [ffi.DeviceBuffer((R, 6)) for _ in range(3)] + [ffi.DeviceBuffer((R, 17, 3)), ffi.DeviceBuffer((R, 8), np.float64)]
    ffi.p2s_fit(dev(np.asarray(k, np.float32)), dev(np.asarray(roi_img, np.int32)), R, dev(m1s(hws)), dev(np.asarray(tp, np.float32)), len(tp),
                align_corners, *outs)
    return [o.numpy() for o in outs]


def align_skeleton(ffi, feat, roi_img, G, kal, out_c, skeleton=True, fill=np.nan):
    """feat [N, Hf, Wf, C] -> [R, 64, 64, out_c]; the skeleton into [C, C + 64) when asked"""
    N, Hf, Wf, C = feat.shape
    R = len(G)
    out = dev(np.full((R, 64, 64, out_c), fill, np.float32))
    ffi.p2s_align(dev(feat), Hf, Wf, C, dev(np.asarray(roi_img, np.int32)), dev(np.asarray(G, np.float32)), R, out, out_c)
    if skeleton:
        ffi.p2s_skeleton(dev(np.asarray(kal, np.float32)), R, out, out_c, C)
    return out.numpy()


def masks(ffi, logits, mmask, counts, hw, K):
    """-> masks [N, K, Hmax, Wmax], boxes [N, K, 4], scores, labels, count"""
    counts = np.asarray(counts, np.int32)
    hw = np.asarray(hw, np.int32).reshape(-1, 2)
    N = len(counts)
    roi_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    Hm, Wm = int(hw[:, 0].max()), int(hw[:, 1].max())
    lg = np.asarray(logits, np.float32) if len(logits) else np.zeros((1, 64, 64, 2), np.float32)
    mm = np.asarray(mmask, np.float32) if len(mmask) else np.zeros((1, 6), np.float32)
    m = dev(np.full((N, K, Hm, Wm), 7, np.uint8))
    b, s = ffi.DeviceBuffer((N, K, 4)), ffi.DeviceBuffer((N, K))
    l, c, ws = ffi.DeviceBuffer((N, K), np.int32), ffi.DeviceBuffer((N,), np.int32), ffi.DeviceBuffer((N, K, 4), np.int32)
    ffi.p2s_masks(dev(lg), dev(mm), dev(counts), dev(roi_off), dev(hw), N, K, Hm, Wm, ws, m, b, s, l, c)
    return m.numpy(), b.numpy(), s.numpy(), l.numpy(), c.numpy()
