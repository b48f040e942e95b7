"""Grouped 3x3 convolution, the parts that need no GPU: the per-group reference of tests/conv_grouped_ref.py against the fp64 formula, the proof that the
isolation inputs tell a zero-padded dense evaluation from a grouped one, the host-side weight packing, and the argument checks of the three entry points."""
import ctypes as C

import numpy as np
import pytest

import conv_grouped_ref as gr
import conv_ref as ref

# every cg x both strides, small: (N, H, W, C, groups, stride)
REF_CASES = [(1, 7, 9, 64, 8, s) for s in (1, 2)] + [(1, 6, 7, 64, 4, s) for s in (1, 2)] + [(1, 5, 8, 64, 2, s) for s in (1, 2)] + \
            [(1, 6, 5, 64, 1, s) for s in (1, 2)] + [(2, 5, 6, 128, 16, 2)]


@pytest.mark.parametrize("case", REF_CASES)
def test_per_group_reference_equals_fp64_of_the_block_diagonal_expansion(case):
    ops = gr.exact_operands(case)
    for act, use_res in gr.VARIANTS:
        sc, sh, rs = gr.form(ops, act, use_res)
        got = gr.grouped_ref(ops["x"], ops["w"], case[4], case[5], sc, sh, rs, act)
        want = ref.expected_f32(gr.fp64_value(case, ops, act, use_res))
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), (case, act, use_res)
        assert len(np.unique(want)) >= 20, "degenerate case"


def test_every_cg_is_covered():
    assert {c[3] // c[4] for c in REF_CASES} == {8, 16, 32, 64} == {c[3] // c[4] for c in gr.CASES}
    assert {c[5] for c in gr.CASES} == {1, 2}


@pytest.mark.parametrize("value", gr.NONFINITE)
def test_isolation_inputs_discriminate(value):
    """One non-finite activation in one channel of one group: the dense oracle on block-diagonal zero-padded weights spreads it into the other groups
    (inf * 0 = NaN), the per-group reference does not.  So the GPU isolation test cannot be passed by a zero-padded dense kernel."""
    from oracle import ora
    case = (1, 6, 7, 64, 8, 1)
    ops = gr.exact_operands(case, key="iso")
    g, cg = 3, 8
    x = ops["x"].copy()
    n, y, xx = gr.isolation_sites(case)[2]
    x[n, y, xx, g * cg + 5] = value
    reach = ref.reach(gr.dense_case(case), [(n, y, xx)])
    dense = ora.conv2d(x, gr.expand(ops["w"], 8), 1, 1)
    grouped = gr.grouped_ref(x, ops["w"], 8, 1)
    inside = np.zeros(64, bool); inside[g * cg:(g + 1) * cg] = True
    assert (~np.isfinite(dense[..., ~inside])).any(), "the dense evaluation must leak into the neighbouring groups"
    bad = ~np.isfinite(grouped)
    assert not bad[..., ~inside].any()
    assert np.array_equal(bad[..., inside], np.broadcast_to(reach[..., None], bad[..., inside].shape))
    clean = gr.grouped_ref(ops["x"], ops["w"], 8, 1)
    assert np.array_equal(ref.bits(grouped)[~bad], ref.bits(clean)[~bad])


@pytest.mark.parametrize("C_,groups", [(64, 8), (128, 8), (64, 2), (192, 3), (64, 1)])
def test_pack_places_every_weight_exactly_once(C_, groups):
    from isegmi import _ffi
    cg = C_ // groups
    d = _ffi.make_conv_desc(1, 8, 8, C_, C_, 3, 3, 1, 1)
    w = np.arange(C_ * 9 * cg, dtype=np.float32).reshape(C_, 3, 3, cg)
    p = _ffi.pack_conv_weights_grouped(d, groups, w)
    assert p.shape == (w.size,)
    assert np.array_equal(np.sort(p), w.reshape(-1))
    # [tile of 16 channels][tap][k-step][lane = 16 q + i] holds w[16 tile + i][tap][4 step + q]
    p6 = p.reshape(C_ // 16, 9, cg // 4, 4, 16)
    assert np.array_equal(p6.transpose(0, 4, 1, 2, 3).reshape(C_, 3, 3, cg), w)


BAD = {
    "cg = 4": dict(Cin=64, Cout=64, groups=16),
    "Cin != Cout": dict(Cin=64, Cout=128, groups=8),
    "R = 1": dict(Cin=64, Cout=64, groups=8, R=1, S=1),
    "stride 3": dict(Cin=64, Cout=64, groups=8, stride=3),
    "strided output": dict(Cin=64, Cout=64, groups=8, out_pix_stride=128),
    "groups do not divide": dict(Cin=64, Cout=64, groups=3),
    "Cin % 64": dict(Cin=96, Cout=96, groups=3),
    "pad 0": dict(Cin=64, Cout=64, groups=8, pad=0),
    "act 2": dict(Cin=64, Cout=64, groups=8, act=2),
    "forced tile": dict(Cin=64, Cout=64, groups=8, tile=4),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_entry_points_refuse(name):
    """ISEGMI_ERR_ARG (-2) from all three entry points, before anything touches a device (this runs without one)."""
    from isegmi import _ffi
    lib = _ffi.lib()
    kw = dict(R=3, S=3, stride=1, pad=1, act=0, tile=0, out_pix_stride=0)
    kw.update(BAD[name])
    groups = kw.pop("groups")
    d = _ffi.make_conv_desc(1, 8, 8, kw["Cin"], kw["Cout"], kw["R"], kw["S"], kw["stride"], kw["pad"], kw["act"], kw["tile"], 0, 0, kw["out_pix_stride"])
    n = C.c_int64(-1)
    assert lib.isegmi_conv_grouped_packed_floats(C.byref(d), C.c_int(groups), C.byref(n)) == -2
    assert n.value == -1
    assert b"bad argument" in lib.isegmi_last_error()
    buf = np.zeros(128 * 9 * 128, np.float32)
    out = np.full(128 * 9 * 128, 7.0, np.float32)
    assert lib.isegmi_pack_conv_weights_grouped(C.byref(d), C.c_int(groups), buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -2
    assert (out == 7.0).all()
    assert lib.isegmi_op_conv2d_grouped(C.byref(d), C.c_int(groups), None, None, None, None, None, None, None) == -2


def test_supported_set_is_accepted_and_empty_launch_is_a_no_op():
    from isegmi import _ffi
    lib = _ffi.lib()
    for C_, groups in [(64, 8), (128, 8), (256, 8), (512, 8), (64, 1), (2048, 32)]:
        for stride in (1, 2):
            d = _ffi.make_conv_desc(2, 8, 8, C_, C_, 3, 3, stride, 1, 1)
            n = C.c_int64(-1)
            assert lib.isegmi_conv_grouped_packed_floats(C.byref(d), C.c_int(groups), C.byref(n)) == 0
            assert n.value == C_ * 9 * (C_ // groups)
    d = _ffi.make_conv_desc(0, 8, 8, 64, 64, 3, 3, 1, 1)
    assert lib.isegmi_op_conv2d_grouped(C.byref(d), C.c_int(8), None, None, None, None, None, None, None) == 0
