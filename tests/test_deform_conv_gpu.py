"""isegmi_op_deform_conv2d on the device, bit for bit (np.array_equal on the uint32 views) against the oracle's unfused form
(tests/deform_conv_cases.py) AND against the device's own two launches (isegmi_op_deform_im2col / _v1, then isegmi_op_conv2d as a 1x1 over 9 C channels).
The kernel's pixel tile is 64 output pixels (deform_conv_cases.TILE) and its Cout band 64 channels (deform_conv_cases.BAND): the shapes sit below, on
and past the tile, below the band and past it by a part of a band."""
import ctypes as C

import numpy as np
import pytest

import deform_conv_cases as dc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), a.size)


def _fused(ffi, c, **kw):
    return ffi.deform_conv2d(c["x"], c["om"], c["w"], c["stride"], c["scale"], c["shift"], c["residual"], c["act"], **kw)


def _two_launches(ffi, c):
    """The device's unfused form: columns, then the 1x1 over 9 C channels.  -> (output, columns)"""
    im2col = ffi.deform_im2col if c["om"].shape[-1] == 27 else ffi.deform_im2col_v1
    col = im2col(c["x"], c["om"], 3, 3, c["stride"], 1, 1)
    cout = c["w"].shape[0]
    return ffi.conv2d(col, np.ascontiguousarray(c["w"]).reshape(cout, 1, 1, -1), 1, 0, c["scale"], c["shift"], c["residual"], c["act"]), col


@pytest.mark.parametrize("i", range(len(dc.RANDOM_SHAPES)), ids=["N%d_%dx%d_C%d_Cout%d_s%d_m%d_r%d" % s for s in dc.RANDOM_SHAPES])
def test_random_shapes_bit_exact(ffi, i):
    c, ref, col = dc.random_reference(i)
    got = _fused(ffi, c)
    _same(got, ref, "fused vs oracle")
    two, dcol = _two_launches(ffi, c)
    _same(dcol, col, "device columns vs oracle")
    _same(got, two, "fused vs the device's two launches")
    assert np.isfinite(got).all() and (got != 0).any()


@pytest.mark.parametrize("modulated", [True, False])
@pytest.mark.parametrize("kind", dc.CRAFTED)
def test_crafted_offsets_bit_exact(ffi, kind, modulated):
    c, ref, col, want = dc.crafted(kind, modulated)
    two, dcol = _two_launches(ffi, c)
    # the condition: the device sampled as many all-zero (pixel, tap) rows as the geometry says -- the case left the image where it was built to
    assert dc.zero_rows(dcol, dc.CC) == want == dc.dead_rows(c["om"], dc.CH, dc.CW, 1)
    _same(dcol, col, "device columns vs oracle")
    got = _fused(ffi, c)
    _same(got, ref, "fused vs oracle")
    _same(got, two, "fused vs the device's two launches")
    if want == dc.CH * dc.CW * 9:   # every tap of every pixel outside: the output is shift, then the activation
        _same(got, np.broadcast_to(np.maximum(c["shift"], np.float32(0)), got.shape), "all outside -> act(shift)")
    if kind == "one_pixel_all_out":
        _same(got[0, 2, 3], np.maximum(c["shift"], np.float32(0)), "the dead pixel")


@pytest.mark.parametrize("modulated", [True, False])
def test_nonfinite_features_under_a_zero_weight_follow_the_reference(ffi, modulated):
    c, ref, col = dc.nonfinite_features(modulated)
    got = _fused(ffi, c)
    assert np.isnan(ref).any() and np.isfinite(ref).any()
    _same(got, ref, "fused vs oracle")
    _same(got, _two_launches(ffi, c)[0], "fused vs the device's two launches")


def test_second_launch_gives_the_same_bits(ffi):
    c, ref, col = dc.random_reference(len(dc.RANDOM_SHAPES) - 8)   # (2, 9, 13) C 256 Cout 260
    _same(_fused(ffi, c, launches=2), ref, "second launch")


def test_unmodulated_equals_modulated_with_a_saturated_mask(ffi):
    c, ref, col = dc.random_reference(5)   # (1, 5, 7) unmodulated
    assert c["om"].shape[-1] == 18
    _same(ffi.deform_conv2d(c["x"], dc.as27(c["om"]), c["w"], c["stride"], c["scale"], c["shift"], c["residual"], c["act"]), ref, "27 channels, +100 logits")


def test_refusals_by_name(ffi):
    """C = 24, C = 544, stride 3, an OC that does not match `modulated`, Cout % 4, null pointers: ISEGMI_ERR_ARG, nothing launched (the poisoned output
    stays as it was); an empty problem is a successful no-op."""
    L = ffi.lib()
    x = ffi.DeviceBuffer.from_numpy(np.ones((1, 4, 4, 544), np.float32))
    om = ffi.DeviceBuffer.from_numpy(np.zeros((1, 4, 4, 27), np.float32))
    w = ffi.DeviceBuffer.from_numpy(np.zeros(128 * 9 * 544, np.float32))
    out = ffi.DeviceBuffer((1, 4, 4, 32)).poison()

    def call(C_=32, OC=27, mod=1, stride=1, Cout=32, px=x, pom=om, pw=w, pout=out, N=1, H=4, W=4):
        return L.isegmi_op_deform_conv2d(ffi._ptr(px), N, H, W, C_, ffi._ptr(pom), OC, mod, stride, ffi._ptr(pw), Cout, None, None, None, 0, ffi._ptr(pout), None)
    for kw, word in ((dict(C_=24), b"multiple of 32"), (dict(C_=544), b"[32, 512]"), (dict(C_=0), b"[32, 512]"), (dict(stride=3), b"stride 1 or 2"),
                     (dict(OC=18), b"27 channels when modulated"), (dict(OC=27, mod=0), b"18 when not"), (dict(OC=26), b"27 channels"),
                     (dict(Cout=30), b"multiple of 4"), (dict(Cout=0), b"multiple of 4"), (dict(mod=2), b"modulated is 0 or 1"),
                     (dict(px=None), b"null device pointer"), (dict(pom=None), b"null device pointer"), (dict(pw=None), b"null device pointer"),
                     (dict(pout=None), b"null device pointer")):
        assert call(**kw) == -2, kw
        msg = L.isegmi_last_error()
        assert b"deform_conv2d" in msg or b"null" in msg, msg
        assert word in msg, (kw, msg)
    poison = out.numpy().view(np.uint8)
    assert (poison == 0xFF).all(), "a refused call must launch nothing"
    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert call(**kw) == 0, kw
    assert call(N=0, px=None, pom=None, pout=None) == 0   # nothing to read or write
    assert (out.numpy().view(np.uint8) == 0xFF).all()
    assert call() == 0
    assert not out.numpy().any()   # zero weights: the launch wrote zeros over the poison
    # the DCNv1 column entry refuses null pointers too
    assert L.isegmi_op_deform_im2col_v1(None, 1, 4, 4, 32, ffi._ptr(om), 3, 3, 1, 1, 1, ffi._ptr(out), None) == -2
