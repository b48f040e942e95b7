"""isegmi_op_box_postprocess with cls_agnostic = 1 (MODEL.CLS_AGNOSTIC_BBOX_REG) against ora.box_postprocess on the tiled regression
-- box_regression[:, -4:] repeated for every class -- bit for bit: the crafted three-proposal input of tests/test_fasterrcnn_cpu.py (on which the
per-class reading gives another answer) and R = 1, 127, 128, 129, 1024 proposals with one crowded class (128 candidates is where a class leaves the
in-block NMS for the bitmask / chip-wide matrix), with the chip-wide crowd workspaces and without."""
import numpy as np
import pytest

import fasterrcnn_cases as fc
from oracle import ora

pytestmark = pytest.mark.gpu


def _compare(ffi, case, chip_wide):
    ncls, (h, w) = case["ncls"], case["hw"]
    R = case["props"].shape[0]
    (gb, gs, gl), = ffi.box_postprocess(case["logits"][None], case["reg8"][None], case["props"][None], np.array([R], np.int32), np.array([[h, w]], np.int32),
                                        chip_wide=chip_wide, cls_agnostic=1)
    rb, rs, rl = ora.box_postprocess(case["logits"], fc.agnostic_regr(case["reg8"], ncls), case["props"], float(w), float(h), cap=100)
    assert np.array_equal(gl, rl) and np.array_equal(gs, rs) and np.array_equal(gb, rb), (R, chip_wide)
    return rb, rs, rl


@pytest.mark.parametrize("chip_wide", [True, False])
def test_class_agnostic_crafted_input_matches_the_tiled_oracle(ffi, chip_wide):
    c = fc.crafted()
    rb, rs, rl = _compare(ffi, c, chip_wide)
    assert len(rs) == 2 and set(rl.tolist()) == {1, 2}
    # the per-class reading of the same rows is another answer (tests/test_fasterrcnn_cpu.py): the kernel did not take it
    pb, ps, pl = ora.box_postprocess(c["logits"], fc.per_class_reading(c["reg8"], c["ncls"]), c["props"], float(c["hw"][1]), float(c["hw"][0]), cap=100)
    assert len(ps) != len(rs)
    # with the field 0 the same memory, as 4 * ncls floats per row, is decoded per class as before
    reg12 = fc.per_class_reading(c["reg8"], c["ncls"])
    (gb, gs, gl), = ffi.box_postprocess(c["logits"][None], reg12[None], c["props"][None], np.array([3], np.int32), np.array([list(c["hw"])], np.int32), chip_wide=chip_wide)
    assert np.array_equal(gl, pl) and np.array_equal(gs, ps) and np.array_equal(gb, pb)


@pytest.mark.parametrize("chip_wide", [True, False])
@pytest.mark.parametrize("R", [1, 127, 128, 129, 1024])
def test_class_agnostic_crowded_class_matches_the_tiled_oracle(ffi, R, chip_wide):
    c = fc.crowded(R)
    # the crowd is real, stated from the reference side: (all but a few of) the proposals are candidates of class 2 -- 128 of 128 stay in the block's own
    # NMS, 129 of 129 are the first to leave it
    z = c["logits"].astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    crowd = int((p[:, 2] > 0.06).sum())
    assert crowd >= R - 2 and (R > 129 or crowd == R)
    rb, rs, rl = _compare(ffi, c, chip_wide)
    assert len(rs) >= 1 and (R < 127 or ((rl == 2).sum() >= 5 and len(rs) < R))   # NMS kept several of the crowded class and suppressed others
