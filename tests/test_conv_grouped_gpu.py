"""isegmi_op_conv2d_grouped against the per-group oracle reference (tests/conv_grouped_ref.py), bit for bit: no tolerance anywhere in this file.  The
contract is one fmaf chain per output over the group's own (r, s, c), so real-valued inputs have ONE right answer too."""
import numpy as np
import pytest

import conv_grouped_ref as gr
import conv_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 4096   # floats of 0xFF behind the output


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not ref.same_bits(got, want):
        bad = np.argwhere(ref.bits(got) != ref.bits(want))
        raise AssertionError("%s: %d of %d differ; first at %s: got %r, want %r" % (what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])],
                                                                                     want[tuple(bad[0])]))


def _run(ffi, case, ops, act, use_res, x=None):
    sc, sh, rs = gr.form(ops, act, use_res)
    out, guard = ffi.conv2d_grouped(ops["x"] if x is None else x, ops["w"], case[4], case[5], sc, sh, rs, act, guard=GUARD)
    assert (guard.view(np.uint32) == 0xFFFFFFFF).all(), "the launch wrote behind its output"
    return out


@pytest.mark.parametrize("case", gr.CASES)
def test_grouped_real_inputs_bit_exact(ffi, case):
    """Real-valued normal inputs: scale, shift, residual and ReLU; and the bare form (act 0, no scale, shift or residual)."""
    ops = gr.real_operands(case)
    for act, use_res in gr.VARIANTS:
        sc, sh, rs = gr.form(ops, act, use_res)
        want = gr.grouped_ref(ops["x"], ops["w"], case[4], case[5], sc, sh, rs, act)
        _same(_run(ffi, case, ops, act, use_res), want, "act %d res %d" % (act, use_res))


@pytest.mark.parametrize("case", gr.CASES)
def test_grouped_exact_inputs(ffi, case):
    """Order-free exact operands against the fp64 value of the block-diagonal expansion."""
    ops = gr.exact_operands(case)
    for act, use_res in gr.VARIANTS:
        want = ref.expected_f32(gr.fp64_value(case, ops, act, use_res))
        _same(_run(ffi, case, ops, act, use_res), want, "act %d res %d" % (act, use_res))


@pytest.mark.parametrize("stride", [1, 2])
def test_one_group_of_64_equals_the_dense_op(ffi, stride):
    case = (1, 34, 34, 64, 1, stride)
    ops = gr.real_operands(case, key="dense")
    for act, use_res in gr.VARIANTS:
        sc, sh, rs = gr.form(ops, act, use_res)
        want = ffi.conv2d(ops["x"], ops["w"], stride, 1, sc, sh, rs, act)
        _same(_run(ffi, case, ops, act, use_res), want, "act %d res %d" % (act, use_res))


# (case, group that gets the non-finite value): cg = 8 with the even and the odd group of a 16-column pair, at both strides; cg = 64
ISOLATION = [((2, 13, 19, 64, 8, 1), 2), ((2, 13, 19, 64, 8, 1), 5), ((1, 17, 9, 128, 16, 2), 6), ((1, 17, 9, 128, 16, 2), 11), ((1, 13, 19, 128, 2, 1), 1)]


@pytest.mark.parametrize("case,group", ISOLATION)
def test_nonfinite_values_stay_inside_their_group(ffi, case, group):
    """+inf, -inf and NaN, one at a time, at a corner, a border and an interior pixel, in one channel of one group: the non-finite outputs are exactly that
    group's cg channels at the positions whose window holds the pixel; every other output is bit-identical to the clean run."""
    C_, groups, stride = case[3], case[4], case[5]
    cg = C_ // groups
    ops = gr.exact_operands(case, key="iso")
    clean = _run(ffi, case, ops, 0, True)
    assert np.isfinite(clean).all()
    inside = np.zeros(C_, bool); inside[group * cg:(group + 1) * cg] = True
    for k, site in enumerate(gr.isolation_sites(case)):
        reach = ref.reach(gr.dense_case(case), [site])
        assert reach.any()
        for value in gr.NONFINITE:
            x = ops["x"].copy()
            x[site[0], site[1], site[2], group * cg + (3 * k + 1) % cg] = value
            got = _run(ffi, case, ops, 0, True, x=x)
            bad = ~np.isfinite(got)
            what = "site %s value %r" % (site, value)
            assert not bad[..., ~inside].any(), what + ": leaked into another group"
            assert np.array_equal(bad[..., inside], np.broadcast_to(reach[..., None], bad[..., inside].shape)), what
            assert np.array_equal(ref.bits(got)[~bad], ref.bits(clean)[~bad]), what
            want = gr.grouped_ref(x, ops["w"], groups, stride, ops["scale"], ops["shift"], ops["residual"], 0)
            assert ref.same_values(got, want), what


def test_refused_arguments_launch_nothing(ffi):
    x = np.zeros((1, 8, 8, 64), np.float32)
    with pytest.raises(ffi.IsegmiError, match="8, 16, 32 or 64"):
        ffi.conv2d_grouped(x, np.zeros((64, 3, 3, 4), np.float32), 16)
