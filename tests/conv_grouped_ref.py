"""Reference, cases and operands of the grouped 3x3 convolution (isegmi_op_conv2d_grouped): numpy and the CPU oracle only.

THE REFERENCE is the oracle's ordered fp32 chain applied PER GROUP: group g = the oracle's dense conv2d on the group's own cg input channels and its own
cg filters, epilogue included (scale, shift and the residual are sliced per group), the results concatenated along the channels.  No output of it ever
meets an input channel of another group.  tests/test_conv_grouped_cpu.py holds it to conv_ref.conv2d_fp64 of the block-diagonal dense expansion on
order-free exact operands, and shows that the OTHER obvious reference -- the dense oracle on the block-diagonal zero-padded weights -- is a different
function on non-finite inputs (inf * 0 = NaN crosses the groups)."""
import numpy as np

import conv_ref as ref
from oracle import ora

# (N, H, W, C, groups, stride): 3x3, pad 1.  The smallest shapes at which the kernel can go wrong: a single pixel; odd and even sizes under stride 2; tiles
# cut on every side (16 output columns x 8 / 4 / 2 output rows per block); one, two, three (not a power of two), four and eight 64-channel slabs; every cg.
CASES = [
    (1, 1, 1, 64, 8, 1),
    (2, 13, 19, 64, 8, 1),
    (1, 2, 37, 128, 8, 1),
    (2, 13, 19, 256, 32, 1),
    (1, 17, 9, 128, 4, 2),
    (1, 16, 10, 128, 2, 2),
    (2, 7, 33, 192, 6, 1),
    (1, 34, 34, 64, 1, 1),
    (1, 9, 70, 512, 32, 2),
]
VARIANTS = ref.VARIANTS   # (act, residual): scale + shift + residual + ReLU, and the bare conv (no scale, no shift, no residual, act 0)


def dense_case(case):
    N, H, W, C, groups, stride = case
    return (N, H, W, C, C, 3, stride, 1)


def expand(w, groups):
    """[C, 3, 3, C / groups] -> the block-diagonal dense [C, 3, 3, C] with zeros outside the groups."""
    C, R, S, cg = w.shape
    assert cg * groups == C
    d = np.zeros((C, R, S, C), w.dtype)
    for g in range(groups):
        d[g * cg:(g + 1) * cg, :, :, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return d


def _slice_w(ops, case):
    """The dense draw's first cg input channels of every filter are the grouped layer's weights."""
    C, groups = case[3], case[4]
    out = dict(ops)
    out["w"] = np.ascontiguousarray(ops["w"][..., :C // groups])
    return out


def exact_operands(case, key=0):
    """Order-free exact operands (conv_ref.exact_operands of the dense case; K only shrinks, so its 2^24 assertion covers the grouped sums)."""
    return _slice_w(ref.exact_operands(dense_case(case), key=("grouped", key)), case)


def real_operands(case, key=0):
    return _slice_w(ref.real_operands(dense_case(case), key=("grouped", key)), case)


def grouped_ref(x, w, groups, stride, scale=None, shift=None, residual=None, act=0):
    """The per-group oracle reference (module docstring)."""
    C = x.shape[3]
    cg = C // groups
    assert w.shape == (C, 3, 3, cg)
    outs = []
    for g in range(groups):
        s = slice(g * cg, (g + 1) * cg)
        outs.append(ora.conv2d(np.ascontiguousarray(x[..., s]), np.ascontiguousarray(w[s]), stride, 1,
                               None if scale is None else np.ascontiguousarray(scale[s]), None if shift is None else np.ascontiguousarray(shift[s]),
                               None if residual is None else np.ascontiguousarray(residual[..., s]), act))
    return np.ascontiguousarray(np.concatenate(outs, axis=3))


def form(ops, act, use_res):
    """Operands of one epilogue form: (scale, shift, residual) or the bare (None, None, None)."""
    return (ops["scale"], ops["shift"], ops["residual"]) if use_res else (None, None, None)


def fp64_value(case, ops, act, use_res):
    sc, sh, rs = form(ops, act, use_res)
    return ref.conv2d_fp64(ops["x"], expand(ops["w"], case[4]), case[5], 1, sc, sh, rs, act)


def isolation_sites(case):
    """A corner, a border and an interior input pixel (n, y, x)."""
    N, H, W = case[:3]
    return [(0, 0, 0), (N - 1, H - 1, W // 2), (N - 1, H // 2, W // 2)]


NONFINITE = [np.inf, -np.inf, np.nan]
