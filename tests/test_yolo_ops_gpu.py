"""The YOLOv3 tail kernels (csrc/yolo_ops.hip) against tests/yolov3_ref.py on the crafted inputs of tests/yolov3_cases.py, bit for bit.
tests/test_yolov3_cpu.py shows on the CPU that each crafted input discriminates the rule it is named for, or reaches the limit it is named for."""
import ctypes as C

import numpy as np
import pytest

import yolov3_cases as yc
import yolov3_ref as yr

pytestmark = pytest.mark.gpu
F32 = np.float32
SELECT = yc.all_select_cases()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _device(ffi, c):
    return ffi.yolo_select(c["heads"], c["strides"], c["anchors"], c["A"], c["top_n"], c["thr"], int(c["multi_label"]), c["min_wh"], c["canvas_w"], c["canvas_h"])


def _check(ffi, c):
    kw = dict(c)
    heads = kw.pop("heads")
    dec, total = yr.select_decode(heads, **kw)
    got, gtotal = _device(ffi, c)
    assert np.array_equal(gtotal, total), (gtotal.tolist(), total.tolist())
    for l in range(len(heads)):
        for n in range(heads[0].shape[0]):
            b, s, lab = dec[l][n]
            gb, gs, gl = got[l][n]
            assert len(gs) == len(s), (l, n, len(gs), len(s))
            assert np.array_equal(gl, lab), (l, n)
            assert np.array_equal(_bits(gs), _bits(s)) and np.array_equal(_bits(gb), _bits(b)), (l, n)
    return total


@pytest.mark.parametrize("name", sorted(SELECT))
def test_yolo_select(ffi, name):
    _check(ffi, SELECT[name])


def test_slice_size_is_the_one_the_cases_use(ffi):
    for Cc in (1, 2, 80, 255):
        assert ffi.yolo_slice_records(Cc) == yc.slice_records(Cc)


def test_yolo_select_is_reproducible(ffi):
    c = SELECT["count_tie_top64"]
    r0, t0 = _device(ffi, c)
    for _ in range(3):
        r, t = _device(ffi, c)
        assert np.array_equal(t, t0)
        for l in range(3):
            for n in range(2):
                assert all(np.array_equal(_bits(x) if x.dtype == F32 else x, _bits(y) if y.dtype == F32 else y) for x, y in zip(r[l][n], r0[l][n]))


def test_yolo_select_refuses_what_it_cannot_hold(ffi):
    c = dict(SELECT["geom_nl1_C2_N1_g0"])
    for bad in (dict(top_n=1025), dict(top_n=0), dict(thr=-1.0), dict(min_wh=float("nan")), dict(multi_label=2)):
        with pytest.raises(ffi.IsegmiError, match="yolo_select"):
            _device(ffi, dict(c, **bad))
    grid = (C.c_int32 * 2)(2, 3)
    assert ffi.lib().isegmi_op_yolo_select_workspace(1, 1, grid, 3, 2, 1025) == -1 and ffi.lib().isegmi_op_yolo_select_workspace(4, 1, grid, 3, 2, 8) == -1
    assert ffi.lib().isegmi_op_yolo_select_workspace(1, 1, grid, 3, 2, 8) > 0


def test_select_then_postprocess(ffi):
    """yolo_select's device outputs straight into retina_postprocess (nseg = 3, seg_len = top_n, plain areas) against the reference's final lists."""
    c = dict(yc.chain_case())
    heads = c.pop("heads")
    _, _, dets = yr.tail(heads, **c)
    N, top_n = heads[0].shape[0], c["top_n"]
    ob, os_, ol, oc, ot = ffi.yolo_select_device(heads, c["strides"], c["anchors"], c["A"], top_n, c["thr"], 1, c["min_wh"], c["canvas_w"], c["canvas_h"])
    wsb = ffi.lib().isegmi_op_retina_postprocess_workspace(N, 3, top_n)
    ws = ffi.DeviceBuffer((wsb,), np.uint8).poison()
    cnt = ffi.DeviceBuffer((N,), np.int32).poison(); box = ffi.DeviceBuffer((N, 100, 4)).poison(); sc = ffi.DeviceBuffer((N, 100)).poison()
    lab = ffi.DeviceBuffer((N, 100), np.int32).poison()
    a = ffi.RetinaPostArgs(N, 3, top_n, 3, 100, 100, 2, 0.4, ob.ptr, os_.ptr, ol.ptr, oc.ptr, ws.ptr, wsb, cnt.ptr, box.ptr, sc.ptr, lab.ptr)
    ffi.check(ffi.lib().isegmi_op_retina_postprocess(C.byref(a), None))
    k, B, S, Lb = cnt.numpy(), box.numpy(), sc.numpy(), lab.numpy()
    for n in range(N):
        rb, rs, rl = dets[n]
        assert k[n] == len(rs) > 0
        assert np.array_equal(_bits(B[n, :k[n]]), _bits(rb)) and np.array_equal(_bits(S[n, :k[n]]), _bits(rs)) and np.array_equal(Lb[n, :k[n]], rl)


@pytest.mark.parametrize("case", yc.concat_cases())
def test_concat_up2x(ffi, case):
    N, hc, wc, cc, cs = case
    rng = np.random.default_rng(sum(case))
    coarse = rng.normal(0, 1, (N, hc, wc, cc)).astype(F32)
    skip = rng.normal(0, 1, (N, 2 * hc, 2 * wc, cs)).astype(F32)
    assert np.array_equal(_bits(ffi.concat_up2x(coarse, skip)), _bits(yr.concat_up2x(coarse, skip)))


def test_concat_up2x_refuses_null_and_bad_sizes_before_any_launch(ffi):
    """The device pointers are made-up addresses nothing dereferences: every call returns before a launch."""
    lib, fake = ffi.lib(), 0x10000
    good = dict(c=fake, N=1, Hc=2, Wc=3, Cc=32, s=fake, Cs=64, o=fake)
    for bad in (dict(c=None), dict(s=None), dict(o=None), dict(N=0), dict(Hc=0), dict(Wc=-1), dict(Cc=0), dict(Cs=0), dict(Cc=48), dict(Cs=40)):
        a = dict(good, **bad)
        assert lib.isegmi_op_concat_up2x(a["c"], a["N"], a["Hc"], a["Wc"], a["Cc"], a["s"], a["Cs"], a["o"], None) != 0
        assert b"concat_up2x" in lib.isegmi_last_error()
