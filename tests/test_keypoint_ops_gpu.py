"""The Keypoint R-CNN tail op by op on the GPU, bit for bit against tests/keypoint_ref.py: isegmi_op_keypoint_decode on the crafted edges of
tests/keypoint_cases.py, isegmi_op_keypoint_heatmap against the shuffle + the existing bilinear op and against the oracle, and the transposed convolution as
isegmi_op_conv2d on the packed weights."""
import numpy as np
import pytest

import keypoint_cases as kc
import keypoint_ref as kr
from conv_ref import same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cap", [7, 1, 100])
def test_keypoint_decode_equals_the_restatement(ffi, cap):
    """cap 7: N = 3 -- the seven small edge cases fill image 0 (count == cap), image 1 has count 0, image 2 the clamped-border case and one detection the
    size of an 800 x 1344 canvas; the heat maps and boxes of every empty slot are NaN, so a slot that is read shows.  cap 1 and 100: one workgroup column
    and many."""
    heat, boxes, count, want_kpt, want_ks = kc.decode_batch(cap)
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    bad = [(n, c) for n in range(boxes.shape[0]) for c in range(cap) if not (same_bits(kpt[n, c], want_kpt[n, c]) and same_bits(ks[n, c], want_ks[n, c]))]
    assert not bad, bad
    for n in range(boxes.shape[0]):                                                # slots at or beyond count: zeros, whatever their maps hold
        assert not kpt[n, count[n]:].any() and not ks[n, count[n]:].any()
    assert int(count.sum()) > 0 and (kpt[0, 0, :, 2] == 1).all()


def test_keypoint_decode_cases_by_name(ffi):
    """What each crafted detection is there for, read off the kernel's own answer."""
    heat, boxes, count, _, _ = kc.decode_batch(7)
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    d = kc.detections()
    names = ("tiny", "1x57", "identity", "55.5x56.25", "tie", "zero", "last")
    at = {k: kpt[0, i] for i, k in enumerate(names)}
    sc = {k: ks[0, i] for i, k in enumerate(names)}
    F = np.float32
    # identity: the resize is the identity, the keypoint is the map's own arg-max and the score its value
    box, m = d["identity"]
    p = m.reshape(-1, 17).argmax(0)
    assert np.array_equal(at["identity"][:, 0], (p % 56).astype(F) + F(0.5) + F(box[0])) and np.array_equal(at["identity"][:, 1], (p // 56).astype(F) + F(0.5) + F(box[1]))
    assert np.array_equal(sc["identity"], m.reshape(-1, 17)[p, np.arange(17)])
    # tie: the upper of the two equal peaks (first in row-major order), although the lower one lies further left
    box, m = d["tie"]
    assert (at["tie"][:, 1] < box[1] + 2 * 28).all() and (at["tie"][:, 0] > box[0] + 2 * 25).all()
    # zero maps: position 0, score 0
    box = np.asarray(d["zero"][0], F)
    w, h, wc, hc = kr.box_sizes(box)
    assert np.array_equal(at["zero"][:, 0], np.full(17, F(0.5) * (w / F(wc)) + box[0])) and np.array_equal(at["zero"][:, 1], np.full(17, F(0.5) * (h / F(hc)) + box[1]))
    assert not sc["zero"].any()
    # last: the bottom-right position
    box = np.asarray(d["last"][0], F)
    w, h, wc, hc = kr.box_sizes(box)
    assert np.array_equal(at["last"][:, 0], np.full(17, (F(wc - 1) + F(0.5)) * (w / F(wc)) + box[0])) and np.array_equal(at["last"][:, 1], np.full(17, (F(hc - 1) + F(0.5)) * (h / F(hc)) + box[1]))
    # 1 x 1: the one position is the box's centre in both axes
    box = np.asarray(d["tiny"][0], F)
    assert np.array_equal(at["tiny"][:, 0], np.full(17, F(0.5) * F(1.0) + box[0])) and np.array_equal(at["tiny"][:, 1], np.full(17, F(0.5) * F(1.0) + box[1]))
    # every channel of the border case has its own column: a wrong channel stride cannot pass
    assert len(set(kpt[2, 0, :, 0].tolist())) == 17 and (kpt[2, 0, :, 1] < d["border"][0][1] + 3).all()


def test_keypoint_decode_refuses_what_it_does_not_hold(ffi):
    heat = np.zeros((1, 65, 65, 2), np.float32)
    with pytest.raises(ffi.IsegmiError, match="heat-map side"):
        ffi.keypoint_decode(heat, np.zeros((1, 1, 4), np.float32), np.ones(1, np.int32))
    with pytest.raises(ffi.IsegmiError, match="keypoints"):
        ffi.keypoint_decode(np.zeros((1, 8, 8, 33), np.float32), np.zeros((1, 1, 4), np.float32), np.ones(1, np.int32))


@pytest.mark.parametrize("R", [1, 3, 100])
@pytest.mark.parametrize("K", [17, 1])
def test_keypoint_heatmap_equals_shuffle_then_bilinear(ffi, R, K):
    rng = np.random.default_rng(R * 100 + K)
    x = rng.standard_normal((R, 14, 14, 4 * K)).astype(np.float32)
    got = ffi.keypoint_heatmap(x, K)
    assert got.shape == (R, 56, 56, K)
    lr = kr.shuffle(x, K)
    assert lr[0, 3, 5, K - 1] == x[0, 1, 2, (2 * 1 + 1) * K + K - 1]                # (2y + py, 2x + px) <- parity (py, px)
    pad = -K % 4                                                                     # the existing op works on channel quads
    lr4 = np.concatenate([lr, np.zeros(lr.shape[:3] + (pad,), np.float32)], 3) if pad else lr
    assert same_bits(got, np.ascontiguousarray(ffi.resize_bilinear(lr4, 56, 56)[..., :K]))
    assert same_bits(got, kr.heatmap(x, K))


def test_transposed_convolution_on_the_packed_weights(ffi):
    """(R 3, 14 x 14, Cin 512, K 17): isegmi_op_conv2d on the packed 3 x 3 weights against the oracle convolution on the same weights (bit-exact by the
    existing contract) and, after the shuffle, against the fp64 transposed convolution (keypoint_ref.conv_transpose2d_fp64, which the CPU tests hold against
    torch.nn.functional.conv_transpose2d) under tests/conv_ref.py's bound for a K = 4 * 512 sum: every output has four live taps, and the five zero taps add
    exact zeros and no rounding, so e = gamma(4 * 512 + 3) * (abs_sum + |bias|) -- conv_ref.bound's formula with the live K in place of the packed layer's 9 * 512."""
    import conv_ref
    from isegmi.maskrcnn import pack_keypoint_deconv
    from oracle import ora
    rng = np.random.default_rng(11)
    cin, nk = 512, 17
    w = (rng.standard_normal((cin, nk, 4, 4)) * np.sqrt(2.0 / (4 * cin))).astype(np.float32)
    b = rng.standard_normal(nk).astype(np.float32)
    x = np.maximum(rng.standard_normal((3, 14, 14, cin)), 0).astype(np.float32)
    w3, b4 = pack_keypoint_deconv(w, b)
    got = ffi.conv2d(x, w3, 1, 1, None, b4)
    assert got.shape == (3, 14, 14, 4 * nk)
    assert same_bits(got, ora.conv2d(x, w3, 1, 1, None, b4))
    want = kr.conv_transpose2d_fp64(x, w, b)
    e = kr.shuffle(conv_ref.gamma(4 * cin + 3) * (conv_ref.abs_sum(x, w3, 1, 1) + np.abs(b4.astype(np.float64))), nk)
    err = np.abs(kr.shuffle(got, nk).astype(np.float64) - want)
    print("transposed convolution vs fp64: max err / bound %.4f" % float((err / e).max()))
    assert (err <= e).all()
