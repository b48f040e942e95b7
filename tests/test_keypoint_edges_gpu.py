"""isegmi_op_keypoint_decode at exact inputs, in every thread layout, at the operator's limits and on non-finite maps.  The inputs and their
expected results come from tests/keypoint_edge_cases.py, which tests/test_keypoint_fp64_cpu.py checks without a GPU.

Which test catches which kernel mistake:
  `seg < nseg` dropped ................................................................. none can: nseg * rows_per >= hc, so a tail thread's ya = seg * rows_per
                                                                                         is >= hc = yb and its loop is empty with or without the test.  A tail
                                                                                         thread that did run rows at or past hc would offer positions outside
                                                                                         the map: test_thread_layout_sweep at wc 3, 65, 85, 86, 129 .. 255
  the sliding window not reloaded at a segment's start ................................. test_thread_layout_sweep, places segment-first-row / -last-row,
                                                                                         and test_exact_inputs at 224 x 56 and 448 x 56 (four segments)
  `x += ncol` replaced by a single pass ................................................ test_thread_layout_sweep, place second-stride (x = 256) at
                                                                                         wc 257 .. 1023, test_exact_inputs at 56 x 448, test_long_boxes
  the wave merge taking the higher position on ties .................................... test_exact_inputs at 224 x 224 and 224 x 56 (against fp64)
  a NaN that never wins ................................................................ test_non_finite_maps
"""
import numpy as np
import pytest

import keypoint_edge_cases as ke
import keypoint_fp64 as k64
from conv_ref import same_bits

pytestmark = pytest.mark.gpu
F = np.float32


def test_exact_inputs_equal_fp64_bit_for_bit(ffi):
    """29 detections whose fp32 chain is exact (integer maps, power-of-two scales): kscore is the fp64 maximum and det.kpt the keypoint formula at the fp64
    first arg-max -- no restatement in between, and no rounding to excuse a difference.  The last two cases hold their maximum at many positions."""
    heat, boxes, count, cases, want_kpt, want_score, nmax = ke.exact_batch()
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    n = len(cases)
    bad = [cases[i][:2] for i in range(n) if not (same_bits(kpt[0, i], want_kpt[i]) and np.array_equal(ks[0, i].astype(np.float64), want_score[i]))]
    assert not bad, bad
    assert not kpt[0, n:].any() and not ks[0, n:].any() and (nmax[-2:] >= 2).all()


def test_thread_layout_sweep_equals_the_restatement(ffi):
    """133 detections, wc x hc over the edges of ncol / nseg / rows_per, with the peaks of 11 channels on the corners, edges, segment edges and the second
    stride's first column: bit for bit."""
    heat, boxes, count, want_kpt, want_ks, _ = ke.sweep_batch()
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    bad = [(hc, wc) for n, hc in enumerate(ke.SWEEP_HC) for c, wc in enumerate(ke.SWEEP_WC)
           if not (same_bits(kpt[n, c], want_kpt[n, c]) and same_bits(ks[n, c], want_ks[n, c]))]
    assert not bad, bad
    assert not kpt[:, len(ke.SWEEP_WC):].any() and not ks[:, len(ke.SWEEP_WC):].any()


def test_general_inputs_within_the_derived_bound_of_fp64(ffi):
    """The same 133 x 17 maps against fp64 under the bound e of tests/keypoint_fp64.py: kscore within e of the fp64 maximum, and the fp64 map at the
    kernel's position (recovered from det.kpt) within 2e of it.  Measured on the MI355X: score 0.0885 of its bound, arg-max gap 0 (the same position on
    every map) -- the figures of the restatement on the CPU, as they must be."""
    heat, boxes, count, _, _, _ = ke.sweep_batch()
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    worst_score = worst_gap = 0.0
    moved = 0
    for n, hc in enumerate(ke.SWEEP_HC):
        for c, wc in enumerate(ke.SWEEP_WC):
            for k in range(ke.K):
                pos = k64.position_of(boxes[n, c], kpt[n, c, k])
                a, b = k64.against_bound(heat[n * ke.SWEEP_CAP + c][:, :, k], hc, wc, ks[n, c, k], pos)
                worst_score, worst_gap, moved = max(worst_score, a), max(worst_gap, b), moved + int(b > 0)
    print("kernel vs fp64 on the sweep: score %.4f of its bound, arg-max gap %.4f of its bound, %d of %d positions differ from the fp64 arg-max"
          % (worst_score, worst_gap, moved, 133 * ke.K))
    assert worst_score <= 1.0 and worst_gap <= 1.0


def test_non_finite_maps_follow_argmax(ffi):
    """np.argmax's contract: the first NaN of the resized map wins and the score is NaN; an inf pixel gives inf or, where inf - inf comes first, NaN.  At
    112 x 112 (two segments, four waves) and 300 x 40 (six segments).  Scores are compared as "NaN in the same places, every other value bit for bit": a
    NaN's sign and payload are the machine's (x86 produces the negative default NaN, the GPU the positive one); keypoints are finite and compared by bits."""
    heat, boxes, count, want_kpt, want_ks, pos = ke.nan_batch()
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    bad = [(ke.NAN_SIZES[n], kind) for n in range(2) for c, kind in enumerate(ke.NAN_KINDS)
           if not (same_bits(kpt[n, c], want_kpt[n, c]) and ke.same_floats(ks[n, c], want_ks[n, c]))]
    assert not bad, bad
    c = ke.NAN_KINDS.index("all-nan")
    for n in range(2):                                                              # position 0: the keypoint lies in the box's first cell
        assert np.isnan(ks[n, c]).all() and (np.abs(kpt[n, c, :, :2] - boxes[n, c, :2]) < 1).all()


@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("s", [1, 2, 3, 64])
def test_heat_map_sides_and_keypoint_counts(ffi, s, k):
    heat, boxes, count, want_kpt, want_ks = ke.limit_batch(s, k)
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    assert same_bits(kpt, want_kpt) and same_bits(ks, want_ks)


def test_grid_limit_65535_rows_and_the_refusal_of_65536(ffi):
    heat, boxes, count, want_kpt, want_ks = ke.grid_batch()
    assert boxes.shape[0] * boxes.shape[1] == 65535
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    assert same_bits(kpt, want_kpt) and same_bits(ks, want_ks)                      # every slot, the empty ones (zeros) included
    with pytest.raises(ffi.IsegmiError, match=r"N \* cap must be 1\.\.65535"):
        ffi.keypoint_decode(np.zeros((65536, 2, 2, 1), F), np.zeros((256, 256, 4), F), np.zeros(256, np.int32))


def test_long_boxes_and_the_cut_at_16384(ffi):
    """16384 x 1 (256 segments of 64 rows), 1 x 16384 (64 strides) and a box 20000 wide, whose resized width is cut at 16384 while cw stays 20000 / 16384"""
    heat, boxes, count, want_kpt, want_ks = ke.long_batch()
    kpt, ks = ffi.keypoint_decode(heat, boxes, count)
    assert same_bits(kpt, want_kpt) and same_bits(ks, want_ks)
