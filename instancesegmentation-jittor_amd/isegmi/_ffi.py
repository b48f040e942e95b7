"""ctypes binding of libisegmi.so (C ABI in include/isegmi.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, an
exception is raised.  Nothing here imports torch, triton or the test oracle.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (RETINA_MAX_LEVELS, BottleneckDesc, BoxPostArgs, CocoMatchArgs, ConvDesc, P2sImage, RetinaPostArgs,  # noqa: F401 (re-exported)
                   RetinaSelectArgs, RleArgs, YolactDetectArgs)

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libisegmi.so")


class IsegmiError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib, LIB_PATH
    if _lib is None:
        if os.environ.get("ISEGMI_LIB"):  # development hook: same-box A/B of two builds of libisegmi.so (tools/ab_f16.sh)
            LIB_PATH = os.environ["ISEGMI_LIB"]
        if not os.path.exists(LIB_PATH):
            raise IsegmiError(
                "libisegmi.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C instancesegmentation-jittor_amd`; there is no CPU fallback" % LIB_PATH)
        loaded = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        missing = _abi.declare(loaded)   # restype / argtypes of the whole C ABI, once: a wrong arity or a float for an integer raises at the call
        if missing:
            raise IsegmiError("%s does not export %s (include/isegmi.h declares it): rebuild the library" % (LIB_PATH, ", ".join(missing)))
        _lib = loaded
    return _lib


def check(rc):
    if rc != 0:
        raise IsegmiError("libisegmi error %d: %s" % (rc, lib().isegmi_last_error().decode(errors="replace")))


def device_count():
    n = C.c_int(0)
    rc = lib().isegmi_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def set_device(i):
    check(lib().isegmi_set_device(i))


def sync():
    check(lib().isegmi_sync())


def set_f16_mfma_shape(shape):
    """0: v_mfma_f32_32x32x16_f16 everywhere; 1: row strips + fused RPN head on v_mfma_f32_16x16x32_f16; 2: persistent tiles too; 3 (default): 1 + the
    144-row tiles (process-wide; isegmi_set_f16_mfma_shape).  Results are bit-identical under every setting."""
    check(lib().isegmi_set_f16_mfma_shape(int(shape)))


def get_f16_mfma_shape():
    v = C.c_int()
    check(lib().isegmi_get_f16_mfma_shape(C.byref(v)))
    return v.value


def box_calibrate(ms_per_leg=30.0):
    """{mfma_f32_tflops, mfma_f16_tflops, hbm_copy_gbs} of bare loops on the current device (isegmi_box_calibrate)."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    check(lib().isegmi_box_calibrate(ms_per_leg, C.byref(a), C.byref(b), C.byref(c)))
    return {"mfma_f32_tflops": round(a.value, 1), "mfma_f16_tflops": round(b.value, 1), "hbm_copy_gbs": round(c.value, 1)}


class DeviceBuffer:
    """Owning device allocation with numpy shape/dtype metadata."""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().isegmi_malloc(C.byref(p), self.nbytes))
        self.ptr = p

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.shape, a.dtype)
        if b.nbytes:
            check(lib().isegmi_h2d(b.ptr, a.ctypes.data_as(C.c_void_p), b.nbytes))
        return b

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        check(lib().isegmi_h2d(self.ptr, a.ctypes.data_as(C.c_void_p), self.nbytes))

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            check(lib().isegmi_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out

    def zero(self):
        check(lib().isegmi_memset(self.ptr, 0, self.nbytes))

    def poison(self):
        """0xFF in every byte (NaN as fp16 / fp32, -1 as an integer): an element a kernel never wrote cannot pass as a zero."""
        if self.nbytes:
            check(lib().isegmi_memset(self.ptr, 0xFF, self.nbytes))
        return self

    def free(self):
        if self.ptr is not None and self.ptr.value:
            lib().isegmi_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host memory with a numpy view (`.array`): the source of the engines' asynchronous uploads."""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().isegmi_malloc_host(C.byref(p), self.nbytes))
        self.ptr = p
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(p.value), self.dtype).reshape(self.shape)

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self.array = None
            lib().isegmi_free_host(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(b):
    return None if b is None else b.ptr


def make_conv_desc(N, H, W, Cin, Cout, R, S, stride=1, pad=0, act=0, tile=0, out_div=0, out_img_stride=0,
                   out_pix_stride=0):
    return ConvDesc(N, H, W, Cin, Cout, R, S, stride, pad, act, tile, out_div, out_img_stride, out_pix_stride)


def conv_out_hw(desc):
    ho, wo = C.c_int32(), C.c_int32()
    check(lib().isegmi_conv_out_hw(C.byref(desc), C.byref(ho), C.byref(wo)))
    return ho.value, wo.value


def pack_conv_weights(desc, w_krsc):
    """host: [Cout,R,S,Cin] fp32 -> packed 1-D fp32 array."""
    w = np.ascontiguousarray(w_krsc, np.float32)
    assert w.shape == (desc.Cout, desc.R, desc.S, desc.Cin), (w.shape, desc.Cout, desc.R, desc.S, desc.Cin)
    n = C.c_int64()
    check(lib().isegmi_conv_packed_floats(C.byref(desc), C.byref(n)))
    out = np.empty(n.value, np.float32)
    check(lib().isegmi_pack_conv_weights(C.byref(desc), w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def op_conv2d(desc, d_in, d_wpacked, d_scale=None, d_shift=None, d_residual=None, d_out=None):
    check(lib().isegmi_op_conv2d(C.byref(desc), _ptr(d_in), _ptr(d_wpacked), _ptr(d_scale), _ptr(d_shift),
                                 _ptr(d_residual), _ptr(d_out), None))


def _strided_out(shape, dtype, out_shape, out_offset):
    """The output buffer of the conv wrappers, every byte 0xFF before the launch: the dense result, or (out_shape given) a larger array that the strided
    output mode writes into from element out_offset on.  -> (buffer, address of the first element the kernel is given)."""
    do = DeviceBuffer(shape if out_shape is None else out_shape, dtype).poison()
    return do, C.c_void_p(do.ptr.value + int(out_offset) * do.dtype.itemsize)


def conv2d(x, w_krsc, stride=1, pad=0, scale=None, shift=None, residual=None, act=0, tile=0, out_shape=None, out_div=0, out_img_stride=0,
           out_pix_stride=0, out_offset=0):
    """Convenience host->device->host convolution (tests / small inputs).  out_shape: the strided output mode of isegmi_conv_desc -- the whole array
    of that shape is returned, 0xFF in every byte the kernel did not write; result element (m, co) lies at flat index
    out_offset + (m / out_div) * out_img_stride + (m % out_div) * out_pix_stride + co."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cin = x.shape
    Cout, R, S, _ = w_krsc.shape
    d = make_conv_desc(N, H, W, Cin, Cout, R, S, stride, pad, act, tile, out_div, out_img_stride, out_pix_stride)
    ho, wo = conv_out_hw(d)
    dx = DeviceBuffer.from_numpy(x)
    dw = DeviceBuffer.from_numpy(pack_conv_weights(d, w_krsc))
    ds = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dh = None if shift is None else DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    dr = None if residual is None else DeviceBuffer.from_numpy(np.asarray(residual, np.float32))
    do, first = _strided_out((N, ho, wo, Cout), np.float32, out_shape, out_offset)
    check(lib().isegmi_op_conv2d(C.byref(d), dx.ptr, dw.ptr, _ptr(ds), _ptr(dh), _ptr(dr), first, None))
    return do.numpy()


def pack_conv_weights_grouped(desc, groups, w):
    """host: [Cout,3,3,Cin/groups] fp32 -> the packed 1-D fp32 image of isegmi_op_conv2d_grouped."""
    w = np.ascontiguousarray(w, np.float32)
    n = C.c_int64()
    check(lib().isegmi_conv_grouped_packed_floats(C.byref(desc), groups, C.byref(n)))
    assert w.shape == (desc.Cout, 3, 3, desc.Cin // groups), (w.shape, desc.Cout, desc.Cin, groups)
    out = np.empty(n.value, np.float32)
    check(lib().isegmi_pack_conv_weights_grouped(C.byref(desc), groups, w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def op_conv2d_grouped(desc, groups, d_in, d_wpacked, d_scale=None, d_shift=None, d_residual=None, d_out=None):
    check(lib().isegmi_op_conv2d_grouped(C.byref(desc), groups, _ptr(d_in), _ptr(d_wpacked), _ptr(d_scale), _ptr(d_shift),
                                         _ptr(d_residual), _ptr(d_out), None))


def conv2d_grouped(x, w, groups, stride=1, scale=None, shift=None, residual=None, act=0, guard=0):
    """Convenience host->device->host grouped 3x3 / pad 1 convolution (tests / small inputs): x [N,H,W,C], w [C,3,3,C/groups].  guard > 0: the output
    buffer gets that many floats of 0xFF bytes behind it, and (output, guard region after the launch) is returned."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cin = x.shape
    d = make_conv_desc(N, H, W, Cin, w.shape[0], w.shape[1], w.shape[2], stride, 1, act)
    dw = DeviceBuffer.from_numpy(pack_conv_weights_grouped(d, groups, w))
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dx = DeviceBuffer.from_numpy(x)
    ds = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dh = None if shift is None else DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    dr = None if residual is None else DeviceBuffer.from_numpy(np.asarray(residual, np.float32))
    n_out = N * ho * wo * Cin
    do = DeviceBuffer((n_out + int(guard),)).poison()
    op_conv2d_grouped(d, groups, dx, dw, ds, dh, dr, do)
    flat = do.numpy()
    out = flat[:n_out].reshape(N, ho, wo, Cin)
    return (out, flat[n_out:]) if guard else out


def conv2d_group(items):
    """isegmi_op_conv2d_group: several independent fp32 convolutions as ONE launch.  items: dicts with x, w (KRSC) and optionally stride, pad, scale,
    shift, residual, act.  -> list of outputs (each what conv2d gives for the member alone, bit for bit)."""
    n = len(items)
    descs = (ConvDesc * n)()
    keep, ins, ws, scs, shs, rss, outs, shapes = [], [], [], [], [], [], [], []
    for i, it in enumerate(items):
        x = np.ascontiguousarray(it["x"], np.float32)
        N, H, W, Cin = x.shape
        Cout, R, S, _ = it["w"].shape
        d = make_conv_desc(N, H, W, Cin, Cout, R, S, it.get("stride", 1), it.get("pad", 0), it.get("act", 0), 0)
        descs[i] = d
        ho, wo = conv_out_hw(d)
        dx = DeviceBuffer.from_numpy(x); dw = DeviceBuffer.from_numpy(pack_conv_weights(d, it["w"]))
        ds = None if it.get("scale") is None else DeviceBuffer.from_numpy(np.asarray(it["scale"], np.float32))
        dh = None if it.get("shift") is None else DeviceBuffer.from_numpy(np.asarray(it["shift"], np.float32))
        dr = None if it.get("residual") is None else DeviceBuffer.from_numpy(np.asarray(it["residual"], np.float32))
        do = DeviceBuffer((N, ho, wo, Cout))
        keep += [dx, dw, ds, dh, dr, do]
        for lst, b in ((ins, dx), (ws, dw), (scs, ds), (shs, dh), (rss, dr), (outs, do)):
            lst.append(None if b is None else b.ptr.value)
    arr = lambda lst: (C.c_void_p * n)(*lst)
    check(lib().isegmi_op_conv2d_group(n, descs, arr(ins), arr(ws), arr(scs), arr(shs), arr(rss), arr(outs), None))
    return [keep[6 * i + 5].numpy() for i in range(n)]


def maxpool(x, k, s, p):
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cc = x.shape
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, ho, wo, Cc)).poison()
    check(lib().isegmi_op_maxpool(dx.ptr, N, H, W, Cc, k, s, p, do.ptr, None))
    return do.numpy()


def maxpool_f16(x, k, s, p, in_f16=True):
    """isegmi_op_maxpool_f16: x [N,H,W,C] cast to fp16 (fp32 when not in_f16) -> fp16 [N,Ho,Wo,C]."""
    x = np.ascontiguousarray(x, np.float16 if in_f16 else np.float32)
    N, H, W, Cc = x.shape
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, max(ho, 0), max(wo, 0), Cc), np.float16).poison()
    check(lib().isegmi_op_maxpool_f16(dx.ptr, int(bool(in_f16)), N, H, W, Cc, k, s, p, do.ptr, None))
    return do.numpy()


def resize_bilinear(x, Ho, Wo, add=None, relu=0):
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, Ho, Wo, Cc)).poison()
    da = None if add is None else DeviceBuffer.from_numpy(np.asarray(add, np.float32))
    check(lib().isegmi_op_resize_bilinear(dx.ptr, N, H, W, Cc, Ho, Wo, _ptr(da), relu, do.ptr, None))
    return do.numpy()


def keypoint_heatmap(x, K):
    """isegmi_op_keypoint_heatmap: x [R, Hi, Wi, 4 * K] (the packed transposed convolution's output) -> [R, 4 Hi, 4 Wi, K]."""
    x = np.ascontiguousarray(x, np.float32)
    R, Hi, Wi, c = x.shape
    assert c == 4 * K, (c, K)
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((R, 4 * Hi, 4 * Wi, K)).poison()
    check(lib().isegmi_op_keypoint_heatmap(dx.ptr, R, Hi, Wi, K, do.ptr, None))
    return do.numpy()


def keypoint_decode(heat, boxes, count):
    """isegmi_op_keypoint_decode: heat [N * cap, S, S, K], boxes [N, cap, 4], count [N] -> (kpt [N, cap, K, 3], kscore [N, cap, K])."""
    heat = np.ascontiguousarray(heat, np.float32)
    boxes = np.ascontiguousarray(boxes, np.float32)
    count = np.ascontiguousarray(count, np.int32)
    N, cap = boxes.shape[:2]
    R, S, S2, K = heat.shape
    assert R == N * cap and S == S2 and boxes.shape == (N, cap, 4) and count.shape == (N,), (heat.shape, boxes.shape, count.shape)
    dh, db, dc = DeviceBuffer.from_numpy(heat), DeviceBuffer.from_numpy(boxes), DeviceBuffer.from_numpy(count)
    dk, ds = DeviceBuffer((N, cap, K, 3)).poison(), DeviceBuffer((N, cap, K)).poison()
    check(lib().isegmi_op_keypoint_decode(dh.ptr, db.ptr, dc.ptr, N, cap, S, K, dk.ptr, ds.ptr, None))
    return dk.numpy(), ds.numpy()


def resize_bilinear_f16(x, Ho, Wo, add=None, relu=0):
    """isegmi_op_resize_bilinear_f16: x [N,H,W,C] and add [N,Ho,Wo,C] cast to fp16 -> fp16 [N,Ho,Wo,C]."""
    x = np.ascontiguousarray(x, np.float16)
    N, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, Ho, Wo, Cc), np.float16).poison()
    da = None if add is None else DeviceBuffer.from_numpy(np.ascontiguousarray(add, np.float16))
    assert da is None or da.shape == do.shape, (da.shape, do.shape)
    check(lib().isegmi_op_resize_bilinear_f16(dx.ptr, N, H, W, Cc, Ho, Wo, _ptr(da), int(relu), do.ptr, None))
    return do.numpy()


def preprocess_u8(images_u8, Hout, Wout, Hpad, Wpad, mean3, std3, swap_rb):
    """isegmi_op_preprocess_u8 (the device front end, M1 / Y1): [N, Hin, Win, 3] uint8 -> [N, Hpad, Wpad, 3] fp32."""
    x = np.ascontiguousarray(images_u8)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise TypeError("preprocess_u8 takes an [N, H, W, 3] uint8 batch")
    N, H, W, _ = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, Hpad, Wpad, 3))
    m = (C.c_float * 3)(*[float(v) for v in mean3]); sd = (C.c_float * 3)(*[float(v) for v in std3])
    check(lib().isegmi_op_preprocess_u8(dx.ptr, N, H, W, do.ptr, Hout, Wout, Hpad, Wpad, Hpad * Wpad * 3, m, sd, int(bool(swap_rb)), None))
    return do.numpy()


def preprocess_u8_flip(images_u8, Hout, Wout, Hpad, Wpad, mean3, std3, swap_rb, hflip):
    """isegmi_op_preprocess_u8_flip: preprocess_u8 of the images mirrored within their own width, the bytes untouched."""
    x = np.ascontiguousarray(images_u8)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise TypeError("preprocess_u8_flip takes an [N, H, W, 3] uint8 batch")
    N, H, W, _ = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, Hpad, Wpad, 3)).poison()
    m = (C.c_float * 3)(*[float(v) for v in mean3]); sd = (C.c_float * 3)(*[float(v) for v in std3])
    check(lib().isegmi_op_preprocess_u8_flip(dx.ptr, N, H, W, do.ptr, Hout, Wout, Hpad, Wpad, Hpad * Wpad * 3, m, sd, int(bool(swap_rb)), int(bool(hflip)), None))
    return do.numpy()


def resample_tile():
    """(tile rows, tile columns, source rows per LDS chunk) of isegmi_op_resample_u8's kernel."""
    th, tw, rc = C.c_int(), C.c_int(), C.c_int()
    check(lib().isegmi_op_resample_tile(C.byref(th), C.byref(tw), C.byref(rc)))
    return th.value, tw.value, rc.value


def resample_u8(images, entries, canvas=None, planes=None, mean3=(0, 0, 0), std3=(1, 1, 1), swap_rb=False, fill=0.0):
    """isegmi_op_resample_u8, one launch: images = HxWx3 uint8 arrays, packed back to back in one blob behind their tables
    (transforms.ResamplePlan); entries = (image, Hout, Wout, dst_y, dst_x, hflip, plane) per resized view.  canvas = (Hpad, Wpad): -> fp32
    [planes, Hpad, Wpad, 3], every canvas element of every plane an entry names written (normalised pixel or `fill`); canvas None: -> the
    resized uint8 images, tight.  Both outputs are poisoned (0xFF bytes: NaN / 255) before the launch."""
    from .transforms import ResamplePlan
    ims = [np.ascontiguousarray(im) for im in images]
    plan = ResamplePlan([im.shape[:2] for im in ims], [entries])
    blob = np.empty(plan.nbytes, np.uint8)
    plan.write(blob, ims)
    table = plan.header()[1][0].copy()
    out_off, off = [], 0
    for r in range(table.shape[0]):   # the byte outputs back to back (words 14, 15; all far below 2^31 here)
        out_off.append(off)
        table[r, 14] = off
        off += int(table[r, 4]) * int(table[r, 5]) * 3
    blob[:table.nbytes] = table.reshape(-1).view(np.uint8)
    db = DeviceBuffer.from_numpy(blob)
    base = db.ptr.value
    m = (C.c_float * 3)(*[float(v) for v in mean3]); sd = (C.c_float * 3)(*[float(v) for v in std3])
    try:
        if canvas is not None:
            Hp, Wp = canvas
            P = int(planes if planes is not None else 1 + max(int(e[6]) for e in entries))
            do = DeviceBuffer((P, Hp, Wp, 3)).poison()
            args = (do.ptr, P, Hp, Wp, Hp * Wp * 3, m, sd, int(bool(swap_rb)), float(fill), None, 0)
        else:
            do = DeviceBuffer((max(off, 1),), np.uint8).poison()
            args = (None, 0, 0, 0, 0, None, None, 0, 0.0, do.ptr, off)
        try:
            check(lib().isegmi_op_resample_u8(C.c_void_p(base + plan.src_off), plan.pixel_bytes, C.c_void_p(base), table.ctypes.data_as(C.c_void_p), table.shape[0],
                                              C.c_void_p(base + plan.coeff_off), plan.coeff_words, *args, None))
            check(lib().isegmi_sync())
            out = do.numpy()
        finally:
            do.free()
    finally:
        db.free()
    if canvas is not None:
        return out
    return [out[o:o + int(t[4]) * int(t[5]) * 3].reshape(int(t[4]), int(t[5]), 3).copy() for o, t in zip(out_off, table)]


def deform_im2col(x, om, R=3, S=3, stride=1, pad=1, dil=1):
    """x [N,H,W,C], om [N,Ho,Wo,3*R*S] raw conv_offset_mask output -> DCNv2 columns [N,Ho,Wo,R*S*C]."""
    x = np.ascontiguousarray(x, np.float32); om = np.ascontiguousarray(om, np.float32)
    N, H, W, Cc = x.shape
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    assert om.shape == (N, Ho, Wo, 3 * R * S), om.shape
    dx = DeviceBuffer.from_numpy(x); dm = DeviceBuffer.from_numpy(om); do = DeviceBuffer((N, Ho, Wo, R * S * Cc))
    check(lib().isegmi_op_deform_im2col(dx.ptr, N, H, W, Cc, dm.ptr, R, S, stride, pad, dil, do.ptr, None))
    return do.numpy()


def deform_im2col_v1(x, off, R=3, S=3, stride=1, pad=1, dil=1):
    """x [N,H,W,C], off [N,Ho,Wo,2*R*S] raw offset-conv output -> DCNv1 columns [N,Ho,Wo,R*S*C] (no mask factor)."""
    x = np.ascontiguousarray(x, np.float32); off = np.ascontiguousarray(off, np.float32)
    N, H, W, Cc = x.shape
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    assert off.shape == (N, Ho, Wo, 2 * R * S), off.shape
    dx = DeviceBuffer.from_numpy(x); dm = DeviceBuffer.from_numpy(off); do = DeviceBuffer((N, Ho, Wo, R * S * Cc))
    check(lib().isegmi_op_deform_im2col_v1(dx.ptr, N, H, W, Cc, dm.ptr, R, S, stride, pad, dil, do.ptr, None))
    return do.numpy()


def deform_conv2d(x, om, w_krsc, stride=1, scale=None, shift=None, residual=None, act=0, launches=1):
    """isegmi_op_deform_conv2d, host -> device -> host: x [N,H,W,C], om [N,Ho,Wo,27] (DCNv2) or [N,Ho,Wo,18] (DCNv1), w [Cout,3,3,C].  The weights go in
    as the packed image of the 1x1 / 9*C descriptor.  launches > 1: the same launch again into the same (re-poisoned) buffer; the last result returns."""
    x = np.ascontiguousarray(x, np.float32); om = np.ascontiguousarray(om, np.float32)
    N, H, W, Cc = x.shape
    Cout = w_krsc.shape[0]
    Ho, Wo = (H - 1) // stride + 1 if H else 0, (W - 1) // stride + 1 if W else 0
    OC = om.shape[-1]
    d = make_conv_desc(max(N, 1), max(Ho, 1), max(Wo, 1), 9 * Cc, Cout, 1, 1)
    dw = DeviceBuffer.from_numpy(pack_conv_weights(d, np.ascontiguousarray(w_krsc, np.float32).reshape(Cout, 1, 1, 9 * Cc)))
    dx = DeviceBuffer.from_numpy(x); dm = DeviceBuffer.from_numpy(om)
    ds = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dh = None if shift is None else DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    dr = None if residual is None else DeviceBuffer.from_numpy(np.asarray(residual, np.float32))
    do = DeviceBuffer((N, Ho, Wo, Cout))
    for _ in range(launches):
        do.poison()
        check(lib().isegmi_op_deform_conv2d(dx.ptr, N, H, W, Cc, dm.ptr, OC, int(OC == 27), stride, dw.ptr, Cout, _ptr(ds), _ptr(dh), _ptr(dr), act,
                                            do.ptr, None))
    return do.numpy()


def upsample_nearest2x_add(coarse, lateral):
    coarse = np.ascontiguousarray(coarse, np.float32); lateral = np.ascontiguousarray(lateral, np.float32)
    N, Hc, Wc, Cc = coarse.shape
    _, H, W, _ = lateral.shape
    dc = DeviceBuffer.from_numpy(coarse); dl = DeviceBuffer.from_numpy(lateral); do = DeviceBuffer(lateral.shape).poison()
    check(lib().isegmi_op_upsample_nearest2x_add(dc.ptr, N, Hc, Wc, Cc, dl.ptr, H, W, do.ptr, None))
    return do.numpy()


def group_norm_device(d_x, N, H, W, Cc, groups, d_gamma, d_beta, eps=1e-5, d_residual=None, relu=False, d_out=None, d_ws=None, ws_bytes=None,
                      alloc_ws=True, offsets=None):
    """isegmi_op_group_norm on DeviceBuffers (d_out None: in place; d_ws None: allocated here when the shape needs one).  Returns the workspace.
    For the launcher's refusals: `ws_bytes` is the workspace size handed over (default: the buffer's), `alloc_ws` False passes a null workspace where
    none is given, `offsets` {"x" | "out" | "gamma" | "beta" | "residual" | "ws": bytes} moves a pointer into its (over-allocated) buffer."""
    need = lib().isegmi_op_group_norm_workspace_bytes(N, H, W, Cc, groups)
    if d_ws is None and need and alloc_ws:
        d_ws = DeviceBuffer((need,), np.uint8)
    off = offsets or {}

    def at(buf, key):
        return C.c_void_p(buf.ptr.value + off[key]) if buf is not None and off.get(key) else _ptr(buf)
    if ws_bytes is None:
        ws_bytes = d_ws.nbytes if d_ws is not None else 0
    check(lib().isegmi_op_group_norm(at(d_x, "x"), N, H, W, Cc, groups, at(d_gamma, "gamma"), at(d_beta, "beta"), float(eps), at(d_residual, "residual"),
                                     int(bool(relu)), at(d_out or d_x, "out"), at(d_ws, "ws"), ws_bytes, None))
    return d_ws


def group_norm(x, groups, gamma, beta, eps=1e-5, residual=None, relu=False, inplace=False):
    """GroupNorm of x [N,H,W,C] fp32 over (H, W, C / groups) per image and group, + residual, ReLU (isegmi_op_group_norm; N may be 0).
    inplace: the kernel writes over its input (same result; the tests run both)."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x)
    dg = DeviceBuffer.from_numpy(np.ascontiguousarray(gamma, np.float32)); db = DeviceBuffer.from_numpy(np.ascontiguousarray(beta, np.float32))
    assert dg.shape == (Cc,) and db.shape == (Cc,), (dg.shape, db.shape, Cc)
    dr = None if residual is None else DeviceBuffer.from_numpy(np.ascontiguousarray(residual, np.float32))
    assert dr is None or dr.shape == x.shape, (dr.shape, x.shape)
    do = dx if inplace else DeviceBuffer(x.shape).poison()
    group_norm_device(dx, N, H, W, Cc, int(groups), dg, db, eps, dr, relu, do)
    return do.numpy()


def upsample_nearest2x_add_f16(coarse, lateral):
    """isegmi_op_upsample_nearest2x_add_f16: coarse [N,Hc,Wc,C], lateral [N,H,W,C] cast to fp16 -> fp16 [N,H,W,C]."""
    coarse = np.ascontiguousarray(coarse, np.float16); lateral = np.ascontiguousarray(lateral, np.float16)
    N, Hc, Wc, Cc = coarse.shape
    N2, H, W, C2 = lateral.shape
    assert (N2, C2) == (N, Cc), (coarse.shape, lateral.shape)
    dc = DeviceBuffer.from_numpy(coarse); dl = DeviceBuffer.from_numpy(lateral); do = DeviceBuffer(lateral.shape, np.float16).poison()
    check(lib().isegmi_op_upsample_nearest2x_add_f16(dc.ptr, N, Hc, Wc, Cc, dl.ptr, H, W, do.ptr, None))
    return do.numpy()


def pad_c3_to_c4(x):
    """isegmi_op_pad_c3_to_c4: [..., 3] fp32 pixels -> [..., 4] with a zero 4th channel."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape[-1] == 3, x.shape
    npix = x.size // 3
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer(x.shape[:-1] + (4,)).poison()
    check(lib().isegmi_op_pad_c3_to_c4(dx.ptr, npix, do.ptr, None))
    return do.numpy()


def map_f32(x, fn):
    x = np.ascontiguousarray(x, np.float32)
    dx = DeviceBuffer.from_numpy(x); dy = DeviceBuffer(x.shape)
    check(lib().isegmi_op_map_f32(dx.ptr, dy.ptr, x.size, fn, None))
    return dy.numpy()


def topk(keys2d, k, limit=None, rows_per_limit=1, row_stride=None):
    """keys2d [rows][n] -> (vals [rows][k], idx [rows][k], cnt [rows]).  row_stride > n: the rows lie row_stride keys apart on the device and the
    row_stride - n keys between them hold +inf (selected first if the kernel ever read them)."""
    keys2d = np.ascontiguousarray(keys2d, np.float32)
    rows, n = keys2d.shape
    row_stride = n if row_stride is None else int(row_stride)
    assert row_stride >= n
    if row_stride > n:
        padded = np.full((rows, row_stride), np.inf, np.float32)
        padded[:, :n] = keys2d
        keys2d = padded
    dk = DeviceBuffer.from_numpy(keys2d)
    dv = DeviceBuffer((rows, k), np.float32); di = DeviceBuffer((rows, k), np.int32); dc = DeviceBuffer((rows,), np.int32)
    dv.zero(); di.zero()
    dl = None if limit is None else DeviceBuffer.from_numpy(np.asarray(limit, np.int32))
    check(lib().isegmi_op_topk(dk.ptr, row_stride, rows, n, k, _ptr(dl), rows_per_limit, dv.ptr, di.ptr, dc.ptr, None))
    return dv.numpy(), di.numpy(), dc.numpy()


def yolact_detect_prepare(conf_logits, loc, mask, priors, conf_thresh=0.05, nms_thresh=0.5, top_k=200, max_det=100, second_threshold=0,
                          nms_mode=0, trad_cap=1024, max_size=550, fused_A=0, return_nms=False):
    """-> (args, bufs): the argument block of isegmi_op_yolact_detect with every buffer uploaded / allocated, for yolact_detect() below and for
    tools that time repeated calls on the same buffers.  conf_logits [N,P,ncls], loc [N,P,4], mask [N,P,md], priors [P,4].
    nms_mode 0 fast NMS, 1 cross-class fast NMS, 2 traditional per-class NMS (trad_cap candidates per class at most, boxes * max_size).
    fused_A > 0: the three head outputs go to the device as ONE per-pixel row buffer [N][P/A][A*4 | A*ncls | A*md] (the engines' fused head layout).
    return_nms: also return (nms_total [N], nms_overflow [N])."""
    conf_logits = np.ascontiguousarray(conf_logits, np.float32)
    loc = np.ascontiguousarray(loc, np.float32); mask = np.ascontiguousarray(mask, np.float32)
    N, P, ncls = conf_logits.shape
    md = mask.shape[-1]
    nc = ncls - 1
    tkw = int(trad_cap) if nms_mode == 2 else top_k
    bufs = dict(
        d_priors=DeviceBuffer.from_numpy(np.asarray(priors, np.float32)),
        d_ws_scoresT=DeviceBuffer((N, nc, P)), d_ws_boxes=DeviceBuffer((N, P, 4)), d_ws_counts=DeviceBuffer((2 * N,), np.int32),
        d_ws_tk_vals=DeviceBuffer((N, nc, tkw)), d_ws_tk_idx=DeviceBuffer((N, nc, tkw), np.int32),
        d_ws_tk_cnt=DeviceBuffer((N, nc), np.int32), d_ws_cand=DeviceBuffer((N, nc, max(tkw, 128))),
        d_ws_fin_vals=DeviceBuffer((N, max_det)), d_ws_fin_idx=DeviceBuffer((N, max_det), np.int32),
        d_ws_fin_cnt=DeviceBuffer((N,), np.int32), d_out_count=DeviceBuffer((N,), np.int32),
        d_out_boxes=DeviceBuffer((N, max_det, 4)), d_out_scores=DeviceBuffer((N, max_det)),
        d_out_classes=DeviceBuffer((N, max_det), np.int32), d_out_coeffs=DeviceBuffer((N, max_det, md)),
        d_out_prior=DeviceBuffer((N, max_det), np.int32))
    a = YolactDetectArgs()   # zero-initialised: every field not set below keeps the default behaviour
    a.N, a.P, a.ncls, a.mask_dim, a.top_k, a.max_det = N, P, ncls, md, top_k, max_det
    a.conf_thresh, a.nms_thresh = conf_thresh, nms_thresh
    if fused_A:
        A = int(fused_A)
        assert P % A == 0
        row = np.concatenate([loc.reshape(N, P // A, A * 4), conf_logits.reshape(N, P // A, A * ncls), mask.reshape(N, P // A, A * md)], -1)
        bufs["d_head"] = DeviceBuffer.from_numpy(np.ascontiguousarray(row))
        a.d_conf = a.d_loc = a.d_mask = bufs["d_head"].ptr
        a.A, a.pix_stride, a.off_loc, a.off_conf, a.off_mask = A, row.shape[-1], 0, A * 4, A * 4 + A * ncls
    else:
        bufs.update(d_conf=DeviceBuffer.from_numpy(conf_logits), d_loc=DeviceBuffer.from_numpy(loc), d_mask=DeviceBuffer.from_numpy(mask))
    if return_nms or nms_mode:
        bufs.update(d_out_nms_total=DeviceBuffer((N,), np.int32), d_out_nms_overflow=DeviceBuffer((N,), np.int32))
    if nms_mode == 1:
        bufs.update(d_ws_cc_scores=DeviceBuffer((N, P)), d_ws_cc_class=DeviceBuffer((N, P), np.int32))
    if nms_mode == 2:
        bufs.update(d_ws_trad_list=DeviceBuffer((1 + N * nc,), np.int32), d_ws_trad_prior=DeviceBuffer((N, nc, 128), np.int32))
    for name, b in bufs.items():
        if name != "d_head":
            setattr(a, name, b.ptr)
    a.second_threshold = int(second_threshold)
    a.nms_mode, a.trad_cap, a.trad_scale = int(nms_mode), int(trad_cap), float(max_size)
    return a, bufs


def yolact_detect(conf_logits, loc, mask, priors, conf_thresh=0.05, nms_thresh=0.5, top_k=200, max_det=100, second_threshold=0,
                  nms_mode=0, trad_cap=1024, max_size=550, fused_A=0, return_nms=False):
    """Host convenience wrapper: conf_logits [N,P,ncls], loc [N,P,4], mask [N,P,md], priors [P,4]; the keywords are yolact_detect_prepare's."""
    a, bufs = yolact_detect_prepare(conf_logits, loc, mask, priors, conf_thresh, nms_thresh, top_k, max_det, second_threshold, nms_mode, trad_cap,
                                    max_size, fused_A, return_nms)
    N = a.N
    check(lib().isegmi_op_yolact_detect(C.byref(a), None))
    cnt = bufs["d_out_count"].numpy()
    out = []
    B, S, Cl, M, Pr = (bufs[k].numpy() for k in ("d_out_boxes", "d_out_scores", "d_out_classes", "d_out_coeffs", "d_out_prior"))
    for n in range(N):
        c = int(cnt[n])
        out.append(dict(box=B[n, :c], score=S[n, :c], cls=Cl[n, :c], mask=M[n, :c], prior=Pr[n, :c]))
    if return_nms:
        return out, bufs["d_ws_boxes"].numpy(), bufs["d_out_nms_total"].numpy(), bufs["d_out_nms_overflow"].numpy()
    return out, bufs["d_ws_boxes"].numpy()


def yolact_coeff_rows(feats, w_krsc, bias, A, rows, counts, row0, pad=1, sentinel=None, scale=None):
    """isegmi_op_yolact_coeff_rows: feats = list of <= 5 [N,H,W,Cin] maps; w_krsc / bias = the whole head layer (>= row0 + 32 A output channels);
    rows [N,max_det,5] int32 (image, level, ho, wo, anchor); counts [N].  -> [N,max_det,32] pre-tanh; slots past the count keep `sentinel` in
    every element (default: 0xFF bytes)."""
    feats = [np.ascontiguousarray(x, np.float32) for x in feats]
    N, Cin = feats[0].shape[0], feats[0].shape[3]
    Cout, R, S, _ = w_krsc.shape
    rows = np.ascontiguousarray(rows, np.int32)
    assert rows.ndim == 3 and rows.shape[0] == N and rows.shape[2] == 5, rows.shape
    max_det = rows.shape[1]
    d = make_conv_desc(1, R, S, Cin, Cout, R, S, 1, 0)
    dw = DeviceBuffer.from_numpy(pack_conv_weights(d, w_krsc))
    db = None if bias is None else DeviceBuffer.from_numpy(np.asarray(bias, np.float32))
    dsc = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dfs = [DeviceBuffer.from_numpy(x) for x in feats]
    ptrs = (C.c_void_p * len(dfs))(*[b.ptr.value for b in dfs])
    hs = (C.c_int32 * len(dfs))(*[x.shape[1] for x in feats]); ws = (C.c_int32 * len(dfs))(*[x.shape[2] for x in feats])
    dr = DeviceBuffer.from_numpy(rows); dc = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    do = DeviceBuffer((N, max_det, 32)).poison() if sentinel is None else DeviceBuffer.from_numpy(np.full((N, max_det, 32), sentinel, np.float32))
    check(lib().isegmi_op_yolact_coeff_rows(len(dfs), ptrs, hs, ws, N, Cin, R, S, pad, dw.ptr, _ptr(dsc), _ptr(db), A, row0, dr.ptr, dc.ptr, max_det,
                                            do.ptr, None))
    return do.numpy()


def yolact_masks(proto, coeffs, boxes, counts, h, w):
    """proto [N,PH,PW,32]; coeffs [N,K,32]; boxes [N,K,4]; counts [N] -> (masks u8 [N,K,h,w], boxes i64 [N,K,4])"""
    proto = np.ascontiguousarray(proto, np.float32)
    N, PH, PW, md = proto.shape
    K = coeffs.shape[1]
    dp = DeviceBuffer.from_numpy(proto); dc = DeviceBuffer.from_numpy(np.asarray(coeffs, np.float32))
    db = DeviceBuffer.from_numpy(np.asarray(boxes, np.float32)); dn = DeviceBuffer.from_numpy(np.asarray(counts, np.int32))
    dlo = DeviceBuffer.from_numpy(np.full((N, K, PH, PW), np.nan, np.float32))   # the workspace arrives dirty: only crop-window pixels may be read back
    dm = DeviceBuffer((N, K, h, w), np.uint8); dm.zero()
    dob = DeviceBuffer((N, K, 4), np.int64)
    check(lib().isegmi_op_yolact_masks(dp.ptr, dc.ptr, db.ptr, dn.ptr, N, PH, PW, md, K, h, w, dlo.ptr, dm.ptr, dob.ptr, None))
    return dm.numpy(), dob.numpy()


def _initial(init, shape, dtype, fill):
    """caller-supplied initial contents of an output buffer (a poison, or what a previous launch left), or `fill` everywhere"""
    if init is None:
        return np.full(shape, fill, dtype)
    a = np.ascontiguousarray(init, dtype)
    assert a.shape == tuple(shape), (a.shape, shape)
    return a


def yolact_masks_win(proto, coeffs, boxes, counts, h, w, image_hw=None, clear=False, dense_lo=False, planes=None, windows=None, ws_lo=None,
                     want_windows=True):
    """isegmi_op_yolact_masks_win: the mask assembly with the engines' forks.  planes [N,K,h,w] u8, windows [N,K,4] i32 and ws_lo [N,K,PH,PW] f32 are
    the buffers' contents BEFORE the launch (default: 0xA5 bytes, -1, NaN) -> (planes, windows or None, ws_lo, boxes i64) after it."""
    proto = np.ascontiguousarray(proto, np.float32)
    N, PH, PW, md = proto.shape
    K = coeffs.shape[1]
    dp = DeviceBuffer.from_numpy(proto); dc = DeviceBuffer.from_numpy(np.asarray(coeffs, np.float32))
    db = DeviceBuffer.from_numpy(np.asarray(boxes, np.float32)); dn = DeviceBuffer.from_numpy(np.asarray(counts, np.int32))
    dlo = DeviceBuffer.from_numpy(_initial(ws_lo, (N, K, PH, PW), np.float32, np.nan))
    dm = DeviceBuffer.from_numpy(_initial(planes, (N, K, h, w), np.uint8, 0xA5))
    dwin = DeviceBuffer.from_numpy(_initial(windows, (N, K, 4), np.int32, -1)) if want_windows else None
    dh = None if image_hw is None else DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32).reshape(N, 2))
    dob = DeviceBuffer((N, K, 4), np.int64)
    check(lib().isegmi_op_yolact_masks_win(dp.ptr, dc.ptr, db.ptr, dn.ptr, N, PH, PW, md, K, h, w, dlo.ptr, dm.ptr, dob.ptr, _ptr(dh), _ptr(dwin),
                                           int(bool(clear)), int(bool(dense_lo)), None))
    sync()
    return dm.numpy(), (dwin.numpy() if want_windows else None), dlo.numpy(), dob.numpy()


def maskiou_conv1(lo, w, b, out=None):
    """lo [NK,PH,PW]; w [8,9]; b [8] -> [NK,Ho,Wo,32] (isegmi_op_maskiou_conv1); `out`: the output buffer's contents before the launch (default NaN)"""
    lo = np.ascontiguousarray(lo, np.float32)
    NK, PH, PW = lo.shape
    Ho, Wo = (PH - 3) // 2 + 1, (PW - 3) // 2 + 1
    dl = DeviceBuffer.from_numpy(lo); dw = DeviceBuffer.from_numpy(np.ascontiguousarray(w, np.float32).reshape(8, 9))
    db = DeviceBuffer.from_numpy(np.ascontiguousarray(b, np.float32).reshape(8))
    do = DeviceBuffer.from_numpy(_initial(out, (NK, Ho, Wo, 32), np.float32, np.nan))
    check(lib().isegmi_op_maskiou_conv1(dl.ptr, NK, PH, PW, dw.ptr, db.ptr, do.ptr, None))
    sync()
    return do.numpy()


def maskiou_rescore(feat, cls, score, count):
    """feat [N,K,HW,C]; cls i32 / score f32 [N,K]; count [N] -> [N,K] (isegmi_op_maskiou_rescore); the output buffer starts as NaN"""
    feat = np.ascontiguousarray(feat, np.float32)
    N, K, HW, Cc = feat.shape
    df = DeviceBuffer.from_numpy(feat); dc = DeviceBuffer.from_numpy(np.ascontiguousarray(cls, np.int32).reshape(N, K))
    ds = DeviceBuffer.from_numpy(np.ascontiguousarray(score, np.float32).reshape(N, K))
    dn = DeviceBuffer.from_numpy(np.ascontiguousarray(count, np.int32).reshape(N))
    do = DeviceBuffer.from_numpy(np.full((N, K), np.nan, np.float32))
    check(lib().isegmi_op_maskiou_rescore(df.ptr, N, K, HW, Cc, dc.ptr, ds.ptr, dn.ptr, do.ptr, None))
    sync()
    return do.numpy()


# ---------------------------------------------------------------- Mask R-CNN op wrappers (tests / small inputs)
NMS_GE, NMS_NO_PLUS_ONE, NMS_INDEX_ORDER = 1, 2, 4   # ISEGMI_NMS_* of include/isegmi.h (SURVEY App. A.6 forks)


def nms(boxes, scores, thr, plus_one=1, ge=0, max_keep=0):
    """boxes [P,n,4], scores [P,n] -> list of kept original indices (score order) per problem."""
    boxes = np.ascontiguousarray(boxes, np.float32); scores = np.ascontiguousarray(scores, np.float32)
    P, n = scores.shape
    db = DeviceBuffer.from_numpy(boxes); ds = DeviceBuffer.from_numpy(scores)
    dk = DeviceBuffer((P, n), np.int32); dc = DeviceBuffer((P,), np.int32)
    check(lib().isegmi_op_nms(db.ptr, ds.ptr, P, n, thr, plus_one, ge, max_keep, dk.ptr, dc.ptr, None))
    k, c = dk.numpy(), dc.numpy()
    return [k[i, : c[i]].copy() for i in range(P)]


def roi_align(feats, scales, rois, counts, PH, PW, sampling=2, k_min=2, fixed_level=-1, aligned=0):
    """feats: list of [N,H,W,C]; rois [N,K,4]; counts [N] -> (out [N*K,PH,PW,C], levels [N,K])"""
    fb = [DeviceBuffer.from_numpy(np.ascontiguousarray(f, np.float32)) for f in feats]
    N, K = rois.shape[:2]
    Cc = feats[0].shape[3]
    ptrs = (C.c_void_p * len(fb))(*[b.ptr.value for b in fb])
    Hs = (C.c_int32 * len(fb))(*[f.shape[1] for f in feats]); Ws = (C.c_int32 * len(fb))(*[f.shape[2] for f in feats])
    sc = (C.c_float * len(fb))(*scales)
    dr = DeviceBuffer.from_numpy(np.ascontiguousarray(rois, np.float32)); dcnt = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    do = DeviceBuffer((N * K, PH, PW, Cc)).poison(); dl = DeviceBuffer((N, K), np.int32); dl.zero()   # NaN where the launch wrote nothing
    check(lib().isegmi_op_roi_align(ptrs, Hs, Ws, sc, len(fb), dr.ptr, dcnt.ptr, N, K, Cc, PH, PW, sampling, aligned, k_min, fixed_level,
                                    do.ptr, dl.ptr, None))
    return do.numpy(), dl.numpy()


def roi_prep(rois, counts, shapes, scales, Cc, PH, PW, k_min=2, f16=False, want_order=True, aligned=0):
    """first launch of the FPN heads' RoIAlign: rois [N,K,4], counts [N], shapes [(H, W)] per level -> (order [N,K] int32 or None, table [N*K, 2*(PH+PW)+1, 4]
    int32): per-RoI sample rows / columns {low byte offset, high byte offset, low weight bits, high weight bits}, then {level index, H, W, layout signature}"""
    N, K = rois.shape[:2]
    dr = DeviceBuffer.from_numpy(np.ascontiguousarray(rois, np.float32)); dcnt = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    do = DeviceBuffer((N, K), np.int32) if want_order else None
    TS = 2 * (PH + PW) + 1
    assert lib().isegmi_op_roi_table_bytes(N, K, PH, PW) == N * K * TS * 16
    dtab = DeviceBuffer.from_numpy(np.full((N * K, TS, 4), -1, np.int32))
    Hs = (C.c_int32 * len(shapes))(*[h for h, _ in shapes]); Ws = (C.c_int32 * len(shapes))(*[w for _, w in shapes])
    sc = (C.c_float * len(scales))(*scales)
    check(lib().isegmi_op_roi_prep(dr.ptr, dcnt.ptr, N, K, Hs, Ws, sc, len(scales), k_min, Cc, PH, PW, 2 if f16 else 4, aligned, do.ptr if do else None, dtab.ptr, None))
    return (do.numpy() if do else None), dtab.numpy()


def roi_align_ordered(feats, scales, rois, counts, PH, PW, order, table, k_min=2, f16=False):
    """second launch: RoIAlign (sampling 2, LevelMapper) from roi_prep's `table`, launched in `order` [N,K] (any permutation of the rows, or None = row order)
    -> out [N*K,PH,PW,C], pre-filled with NaN so that a row the launch did not write shows"""
    dt = np.float16 if f16 else np.float32
    fb = [DeviceBuffer.from_numpy(np.ascontiguousarray(f, dt)) for f in feats]
    N, K = rois.shape[:2]
    Cc = feats[0].shape[3]
    ptrs = (C.c_void_p * len(fb))(*[b.ptr.value for b in fb])
    Hs = (C.c_int32 * len(fb))(*[f.shape[1] for f in feats]); Ws = (C.c_int32 * len(fb))(*[f.shape[2] for f in feats])
    sc = (C.c_float * len(fb))(*scales)
    dr = DeviceBuffer.from_numpy(np.ascontiguousarray(rois, np.float32)); dcnt = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    dord = DeviceBuffer.from_numpy(np.ascontiguousarray(order, np.int32)) if order is not None else None
    dtab = DeviceBuffer.from_numpy(np.ascontiguousarray(table, np.int32))
    do = DeviceBuffer.from_numpy(np.full((N * K, PH, PW, Cc), np.nan, dt))
    fn = lib().isegmi_op_roi_align_f16_ordered if f16 else lib().isegmi_op_roi_align_ordered
    check(fn(ptrs, Hs, Ws, sc, len(fb), dr.ptr, dcnt.ptr, dord.ptr if dord else None, dtab.ptr, N, K, Cc, PH, PW, k_min, do.ptr, None))
    return do.numpy()


def avgpool_full(x):
    """[R,H,W,C] fp32 -> [R,C]: AvgPool2d over the whole window."""
    x = np.ascontiguousarray(x, np.float32)
    R_, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((R_, Cc)).poison()
    check(lib().isegmi_op_avgpool_full(dx.ptr, R_, H * W, Cc, do.ptr, None))
    return do.numpy()


def roi_align_f16(feats, scales, rois, counts, PH, PW, sampling=2, k_min=2, aligned=0):
    """fp16-storage RoIAlign: feats list of [N,H,W,C] (cast to fp16) -> out [N*K,PH,PW,C] fp16."""
    fb = [DeviceBuffer.from_numpy(np.ascontiguousarray(f, np.float16)) for f in feats]
    N, K = rois.shape[:2]
    Cc = feats[0].shape[3]
    ptrs = (C.c_void_p * len(fb))(*[b.ptr.value for b in fb])
    Hs = (C.c_int32 * len(fb))(*[f.shape[1] for f in feats]); Ws = (C.c_int32 * len(fb))(*[f.shape[2] for f in feats])
    sc = (C.c_float * len(fb))(*scales)
    dr = DeviceBuffer.from_numpy(np.ascontiguousarray(rois, np.float32)); dcnt = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    do = DeviceBuffer((N * K, PH, PW, Cc), np.float16).poison()
    check(lib().isegmi_op_roi_align_f16(ptrs, Hs, Ws, sc, len(fb), dr.ptr, dcnt.ptr, N, K, Cc, PH, PW, sampling, aligned, k_min, do.ptr, None))
    return do.numpy()


def box_postprocess(logits, regr, props, prop_cnt, image_hw, score_thr=0.05, nms_thr=0.5, det_per_img=100, nms_flags=0, cap=0, chip_wide=True,
                    cls_agnostic=0):
    """logits [N,R,ncls], regr [N,R,4*ncls], props [N,R,4] -> list of (boxes, scores, labels).  cls_agnostic: regr is [N,R,8] and every class decodes
    regr[..., 4:8] (MODEL.CLS_AGNOSTIC_BBOX_REG).  cap > det_per_img: rows for the detections
    that tie with the det_per_img-th score (upstream's kth-value rule keeps them).  chip_wide: hand the op its optional crowd workspaces (classes
    with more than 128 candidates get their suppression matrix from the whole chip: three launches); False = every class in its own block."""
    logits = np.ascontiguousarray(logits, np.float32)
    N, R, ncls = logits.shape
    cap = max(det_per_img, cap)
    regr = np.ascontiguousarray(regr, np.float32)
    assert regr.shape == (N, R, 8 if cls_agnostic else 4 * ncls), regr.shape
    b = dict(d_logits=DeviceBuffer.from_numpy(logits), d_regr=DeviceBuffer.from_numpy(np.ascontiguousarray(regr, np.float32)),
             d_props=DeviceBuffer.from_numpy(np.ascontiguousarray(props, np.float32)),
             d_prop_cnt=DeviceBuffer.from_numpy(np.ascontiguousarray(prop_cnt, np.int32)),
             d_image_hw=DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32)),
             d_ws_prob=DeviceBuffer((N, R, ncls)), d_ws_cand_scores=DeviceBuffer((N, ncls - 1, R)),
             d_ws_cand_boxes=DeviceBuffer((N, ncls - 1, R, 4)), d_ws_kept_total=DeviceBuffer((N,), np.int32),
             d_ws_top_vals=DeviceBuffer((N, det_per_img)), d_ws_top_idx=DeviceBuffer((N, det_per_img), np.int32),
             d_out_count=DeviceBuffer((N,), np.int32), d_out_boxes=DeviceBuffer((N, cap, 4)), d_out_scores=DeviceBuffer((N, cap)),
             d_out_labels=DeviceBuffer((N, cap), np.int32))
    if chip_wide:   # dirty on purpose: nothing may be read before it is written
        b.update(d_ws_crowd_matrix=DeviceBuffer.from_numpy(np.full((N, ncls - 1, 131072), 0xa5, np.uint8)), d_ws_crowd_keys=DeviceBuffer((N, ncls - 1, R), np.int64),
                 d_ws_crowd_boxes=DeviceBuffer((N, ncls - 1, R, 4)), d_ws_crowd_m=DeviceBuffer.from_numpy(np.full((N, ncls - 1), 777, np.int32)))
    a = BoxPostArgs(N, R, ncls, det_per_img, cap, nms_flags, score_thr, nms_thr, ncls, regr.shape[2],
                    *[b[n].ptr if n in b else None for n, _ in BoxPostArgs._fields_[10:-1]], int(bool(cls_agnostic)))
    check(lib().isegmi_op_box_postprocess(C.byref(a), None))
    cnt = b["d_out_count"].numpy(); B = b["d_out_boxes"].numpy(); S = b["d_out_scores"].numpy(); Lb = b["d_out_labels"].numpy()
    return [(B[i, : cnt[i]], S[i, : cnt[i]], Lb[i, : cnt[i]]) for i in range(N)]


def mask_logits_select(feat, w, b, labels):
    feat = np.ascontiguousarray(feat, np.float32)
    R, HW, Cc = feat.shape
    df = DeviceBuffer.from_numpy(feat); dw = DeviceBuffer.from_numpy(np.ascontiguousarray(w, np.float32))
    db = DeviceBuffer.from_numpy(np.ascontiguousarray(b, np.float32)); dl = DeviceBuffer.from_numpy(np.ascontiguousarray(labels, np.int32))
    do = DeviceBuffer((R, HW)).poison()
    check(lib().isegmi_op_mask_logits_select(df.ptr, R, HW, Cc, dw.ptr, db.ptr, dl.ptr, do.ptr, None))
    return do.numpy()


def mask_logits_select_f16(feat, w, b, labels):
    """isegmi_op_mask_logits_select_f16: feat [R,HW,C] cast to fp16; w [ncls,C], b [ncls] fp32; labels [R] -> fp32 [R,HW]."""
    feat = np.ascontiguousarray(feat, np.float16)
    R, HW, Cc = feat.shape
    df = DeviceBuffer.from_numpy(feat); dw = DeviceBuffer.from_numpy(np.ascontiguousarray(w, np.float32))
    db = DeviceBuffer.from_numpy(np.ascontiguousarray(b, np.float32)); dl = DeviceBuffer.from_numpy(np.ascontiguousarray(labels, np.int32))
    do = DeviceBuffer((R, HW)).poison()
    check(lib().isegmi_op_mask_logits_select_f16(df.ptr, R, HW, Cc, dw.ptr, db.ptr, dl.ptr, do.ptr, None))
    return do.numpy()


def grid_anchors(base, stride, grid_h, grid_w):
    """isegmi_op_grid_anchors: base [A,4] -> [grid_h*grid_w*A, 4], row (y*grid_w + x)*A + a = base[a] + (x, y, x, y) * stride."""
    base = np.ascontiguousarray(base, np.float32)
    A = base.shape[0]
    assert base.shape == (A, 4), base.shape
    db = DeviceBuffer.from_numpy(base); do = DeviceBuffer((grid_h * grid_w * A, 4)).poison()
    check(lib().isegmi_op_grid_anchors(db.ptr, A, int(stride), int(grid_h), int(grid_w), do.ptr, None))
    return do.numpy()


def paste_masks(masks, boxes, counts, im_h, im_w, thr=0.5):
    masks = np.ascontiguousarray(masks, np.float32)
    N, K, M, _ = masks.shape
    dm = DeviceBuffer.from_numpy(masks); db = DeviceBuffer.from_numpy(np.ascontiguousarray(boxes, np.float32))
    dc = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32)); do = DeviceBuffer((N, K, im_h, im_w), np.uint8)
    check(lib().isegmi_op_paste_masks(dm.ptr, db.ptr, dc.ptr, N, K, M, im_h, im_w, thr, do.ptr, None))
    return do.numpy()


def paste_masks_win(masks, boxes, counts, im_h, im_w, thr=0.5, clear=False, planes=None, windows=None, want_windows=True):
    """isegmi_op_paste_masks_win: the paste with the engines' forks.  planes [N,K,im_h,im_w] u8 and windows [N,K,4] i32 are the buffers' contents
    BEFORE the launch (default: 0xA5 bytes, -1) -> (planes, windows or None) after it."""
    masks = np.ascontiguousarray(masks, np.float32)
    N, K, M, _ = masks.shape
    dm = DeviceBuffer.from_numpy(masks); db = DeviceBuffer.from_numpy(np.ascontiguousarray(boxes, np.float32))
    dc = DeviceBuffer.from_numpy(np.ascontiguousarray(counts, np.int32))
    do = DeviceBuffer.from_numpy(_initial(planes, (N, K, im_h, im_w), np.uint8, 0xA5))
    dwin = DeviceBuffer.from_numpy(_initial(windows, (N, K, 4), np.int32, -1)) if want_windows else None
    check(lib().isegmi_op_paste_masks_win(dm.ptr, db.ptr, dc.ptr, N, K, M, im_h, im_w, thr, do.ptr, _ptr(dwin), int(bool(clear)), None))
    sync()
    return do.numpy(), (dwin.numpy() if want_windows else None)


def rpn_level(head, anchors, image_hw, A, pre_nms, post_nms, nms_thr=0.7, min_size=0.0, nms_flags=0, chip_wide=True):
    """head [N,H,W,A*5] fused (A logits, A*4 deltas) -> list of (boxes, scores).  chip_wide: hand the op its optional
    suppression-matrix workspace (two-kernel NMS, pre_nms <= 1024); False = single-block NMS."""
    head = np.ascontiguousarray(head, np.float32)
    N, H, W, CH = head.shape
    HW = H * W
    dh = DeviceBuffer.from_numpy(head); da = DeviceBuffer.from_numpy(np.ascontiguousarray(anchors, np.float32))
    dhw = DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32))
    wp = DeviceBuffer((N, HW * A)); tv = DeviceBuffer((N, pre_nms)); ti = DeviceBuffer((N, pre_nms), np.int32); tc = DeviceBuffer((N,), np.int32)
    ob = DeviceBuffer((N, post_nms, 4)); os_ = DeviceBuffer((N, post_nms)); oc = DeviceBuffer((N,), np.int32)
    wn = DeviceBuffer((N, 131072), np.uint8) if chip_wide and pre_nms <= 1024 else None
    check(lib().isegmi_op_rpn_level(dh.ptr, da.ptr, dhw.ptr, N, HW, A, pre_nms, post_nms, nms_thr, min_size, nms_flags,
                                    wp.ptr, tv.ptr, ti.ptr, tc.ptr, ob.ptr, os_.ptr, oc.ptr, wn.ptr if wn is not None else None, None))
    c = oc.numpy(); B = ob.numpy(); S = os_.numpy()
    return [(B[i, : c[i]], S[i, : c[i]]) for i in range(N)]


def rpn_levels(heads, anchors, image_hw, A, pre_nms, post_nms, nms_thr=0.7, min_size=0.0, nms_flags=0):
    """All FPN levels at once (isegmi_op_rpn_levels): heads[l] [N,H_l,W_l,A*5], anchors[l] [H_l*W_l*A,4] -> per level a list over images of (boxes, scores)."""
    nl = len(heads)
    hs = [np.ascontiguousarray(h, np.float32) for h in heads]
    N = hs[0].shape[0]
    HW = (C.c_int32 * nl)(*[h.shape[1] * h.shape[2] for h in hs])
    dh = [DeviceBuffer.from_numpy(h) for h in hs]; da = [DeviceBuffer.from_numpy(np.ascontiguousarray(a, np.float32)) for a in anchors]
    ph = (C.c_void_p * nl)(*[b.ptr.value for b in dh]); pa = (C.c_void_p * nl)(*[b.ptr.value for b in da])
    dhw = DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32))
    pe, ce = C.c_int64(), C.c_int64()
    check(lib().isegmi_op_rpn_levels_workspace(nl, N, HW, A, pre_nms, C.byref(pe), C.byref(ce)))
    wp = DeviceBuffer((pe.value,)); cv = DeviceBuffer((ce.value,)); ci = DeviceBuffer((ce.value,), np.int32)
    tv = DeviceBuffer((nl, N, pre_nms)); ti = DeviceBuffer((nl, N, pre_nms), np.int32); tc = DeviceBuffer((nl, N), np.int32)
    wn = DeviceBuffer((nl * N, 131072), np.uint8)
    ob = DeviceBuffer((N, nl, post_nms, 4)); os_ = DeviceBuffer((N, nl, post_nms)); oc = DeviceBuffer((N, nl), np.int32)
    check(lib().isegmi_op_rpn_levels(nl, ph, pa, HW, dhw.ptr, N, A, pre_nms, post_nms, nms_thr, min_size, nms_flags, wp.ptr, cv.ptr, ci.ptr,
                                     tv.ptr, ti.ptr, tc.ptr, wn.ptr, ob.ptr, os_.ptr, oc.ptr, None))
    c = oc.numpy(); B = ob.numpy(); S = os_.numpy()
    return [[(B[i, l, : c[i, l]], S[i, l, : c[i, l]]) for i in range(N)] for l in range(nl)]


# ---------------------------------------------------------------- RetinaNet tail
def retina_select(logits, A, top_n, score_thr=0.05, deltas=None, anchors=None, image_hw=None, min_size=0.0):
    """isegmi_op_retina_select: logits[l] [N,H_l,W_l,A*C] -> per level a list over images of (scores, flat indices); with deltas[l] [N,H_l,W_l,A*4],
    anchors[l] [H_l*W_l*A,4] and image_hw [N,2] also the decoded lists: (sel, dec) with dec[l][i] = (boxes, scores, labels)."""
    nl = len(logits)
    lg = [np.ascontiguousarray(x, np.float32) for x in logits]
    N = lg[0].shape[0]
    Cc = lg[0].shape[3] // A
    a = RetinaSelectArgs()
    a.nl, a.N, a.A, a.C, a.top_n = nl, N, A, Cc, top_n
    a.score_thresh, a.min_size = score_thr, min_size
    keep = [DeviceBuffer.from_numpy(x) for x in lg]
    for l in range(nl):
        a.HW[l] = lg[l].shape[1] * lg[l].shape[2]
        a.d_logits[l] = keep[l].ptr.value
    wsb = lib().isegmi_op_retina_select_workspace(nl, N, a.HW, A, Cc, top_n)
    if wsb < 0:
        raise IsegmiError("isegmi_op_retina_select_workspace: bad sizes")
    ws = DeviceBuffer((wsb,), np.uint8).poison()
    a.d_ws, a.ws_bytes = ws.ptr, wsb
    ss = DeviceBuffer((N, nl, top_n)).poison(); si = DeviceBuffer((N, nl, top_n), np.int32).poison(); sc = DeviceBuffer((N, nl), np.int32).poison()
    a.d_sel_scores, a.d_sel_idx, a.d_sel_cnt = ss.ptr, si.ptr, sc.ptr
    dec = deltas is not None
    if dec:
        keep += [DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32)) for x in deltas]
        keep += [DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32)) for x in anchors]
        for l in range(nl):
            a.d_deltas[l] = keep[nl + l].ptr.value
            a.d_anchors[l] = keep[2 * nl + l].ptr.value
        dhw = DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32))
        ob = DeviceBuffer((N, nl * top_n, 4)).poison(); os_ = DeviceBuffer((N, nl * top_n)).poison()
        ol = DeviceBuffer((N, nl * top_n), np.int32).poison(); oc = DeviceBuffer((N, nl), np.int32).poison()
        a.d_image_hw, a.d_out_boxes, a.d_out_scores, a.d_out_labels, a.d_out_cnt = dhw.ptr, ob.ptr, os_.ptr, ol.ptr, oc.ptr
    check(lib().isegmi_op_retina_select(C.byref(a), None))
    c = sc.numpy(); S = ss.numpy(); I = si.numpy()
    assert (S[np.arange(top_n)[None, None, :] >= c[:, :, None]] == -1).all() and (I[np.arange(top_n)[None, None, :] >= c[:, :, None]] == -1).all()
    sel = [[(S[i, l, : c[i, l]], I[i, l, : c[i, l]]) for i in range(N)] for l in range(nl)]
    if not dec:
        return sel
    c = oc.numpy(); B = ob.numpy().reshape(N, nl, top_n, 4); S = os_.numpy().reshape(N, nl, top_n); Lb = ol.numpy().reshape(N, nl, top_n)
    past = np.arange(top_n)[None, None, :] >= c[:, :, None]   # the rows past a count are filled: zero box, score -1, label 0
    assert (S[past] == -1).all() and (Lb[past] == 0).all() and not B[past].any()
    return sel, [[(B[i, l, : c[i, l]], S[i, l, : c[i, l]], Lb[i, l, : c[i, l]]) for i in range(N)] for l in range(nl)]


def retina_postprocess(boxes, scores, labels, seg_cnt, ncls=81, nms_thr=0.4, det_per_img=100, cap=128, nms_flags=0):
    """isegmi_op_retina_postprocess: boxes [N,nseg,seg_len,4], scores / labels [N,nseg,seg_len], seg_cnt [N,nseg] -> list of (boxes, scores, labels)."""
    boxes = np.ascontiguousarray(boxes, np.float32)
    N, nseg, seg_len, _ = boxes.shape
    cap = max(det_per_img, cap)
    db = DeviceBuffer.from_numpy(boxes); ds = DeviceBuffer.from_numpy(np.ascontiguousarray(scores, np.float32))
    dl = DeviceBuffer.from_numpy(np.ascontiguousarray(labels, np.int32)); dc = DeviceBuffer.from_numpy(np.ascontiguousarray(seg_cnt, np.int32))
    wsb = lib().isegmi_op_retina_postprocess_workspace(N, nseg, seg_len)
    if wsb < 0:
        raise IsegmiError("isegmi_op_retina_postprocess_workspace: bad sizes")
    ws = DeviceBuffer((wsb,), np.uint8).poison()   # dirty on purpose: nothing may be read before it is written
    oc = DeviceBuffer((N,), np.int32).poison(); ob = DeviceBuffer((N, cap, 4)).poison(); os_ = DeviceBuffer((N, cap)).poison(); ol = DeviceBuffer((N, cap), np.int32).poison()
    a = RetinaPostArgs(N, nseg, seg_len, ncls, det_per_img, cap, nms_flags, nms_thr, db.ptr, ds.ptr, dl.ptr, dc.ptr, ws.ptr, wsb, oc.ptr, ob.ptr, os_.ptr, ol.ptr)
    check(lib().isegmi_op_retina_postprocess(C.byref(a), None))
    c = oc.numpy(); B = ob.numpy(); S = os_.numpy(); Lb = ol.numpy()
    return [(B[i, : c[i]], S[i, : c[i]], Lb[i, : c[i]]) for i in range(N)]


# ---------------------------------------------------------------- test-time box augmentation
class BBoxAugPool:
    """The per-image candidate pool of isegmi_op_bbox_aug_candidates on the device: boxes [N,cap,4], scores / labels [N,cap], cnt / total [N].  Created
    poisoned (nothing may be read before it is written) with the counters at `cnt` / `total` (default 0)."""

    def __init__(self, N, cap, cnt=None, total=None):
        self.N, self.cap = int(N), int(cap)
        self.boxes = DeviceBuffer((N, cap, 4)).poison(); self.scores = DeviceBuffer((N, cap)).poison(); self.labels = DeviceBuffer((N, cap), np.int32).poison()
        c = np.zeros(N, np.int32) if cnt is None else np.ascontiguousarray(cnt, np.int32)
        self.cnt = DeviceBuffer.from_numpy(c)
        self.total = DeviceBuffer.from_numpy(c.copy() if total is None else np.ascontiguousarray(total, np.int32))

    def numpy(self):
        """-> (boxes, scores, labels, cnt, total) as they are on the device, slots past the counts included"""
        return self.boxes.numpy(), self.scores.numpy(), self.labels.numpy(), self.cnt.numpy(), self.total.numpy()


def bbox_aug_candidates(pool, logits, regr, props, prop_cnt, image_hw, hflip=0, ratios_wh=None, score_thr=0.05, cls_agnostic=0, R=None, ncls=None, cap=None):
    """isegmi_op_bbox_aug_candidates of one view into `pool` (a BBoxAugPool): logits [N,R,ncls], regr [N,R,4*ncls] ([N,R,8] with cls_agnostic), props [N,R,4],
    prop_cnt [N], image_hw [N,2], ratios_wh [N,2] (default 1).  R / ncls / cap override what the arrays say (refusal tests)."""
    logits = np.ascontiguousarray(logits, np.float32); regr = np.ascontiguousarray(regr, np.float32)
    N, R_, C_ = logits.shape
    r = np.ones((N, 2), np.float32) if ratios_wh is None else np.ascontiguousarray(ratios_wh, np.float32).reshape(N, 2)
    dl = DeviceBuffer.from_numpy(logits); dr = DeviceBuffer.from_numpy(regr); dp = DeviceBuffer.from_numpy(np.ascontiguousarray(props, np.float32))
    dc = DeviceBuffer.from_numpy(np.ascontiguousarray(prop_cnt, np.int32)); dh = DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32))
    drt = DeviceBuffer.from_numpy(r)
    wsb = max(int(lib().isegmi_op_bbox_aug_workspace(N, R_)), 256)
    ws = DeviceBuffer((wsb,), np.uint8).poison()
    check(lib().isegmi_op_bbox_aug_candidates(N, R_ if R is None else R, C_ if ncls is None else ncls, int(bool(cls_agnostic)), int(bool(hflip)),
                                              pool.cap if cap is None else cap, score_thr, dl.ptr, C_, dr.ptr, regr.shape[2], dp.ptr, dc.ptr, dh.ptr, drt.ptr, ws.ptr, wsb,
                                              pool.boxes.ptr, pool.scores.ptr, pool.labels.ptr, pool.cnt.ptr, pool.total.ptr, None))
    check(lib().isegmi_sync())


def bbox_aug_merge(pool, ncls, nms_thr=0.5, det_per_img=100, cap=100, nms_flags=0):
    """The merge of test-time box augmentation: isegmi_op_retina_postprocess over the pool with nseg 1, seg_len cap, d_seg_cnt the pool count."""
    N = pool.N
    wsb = lib().isegmi_op_retina_postprocess_workspace(N, 1, pool.cap)
    ws = DeviceBuffer((wsb,), np.uint8).poison()
    cap = max(det_per_img, cap)
    oc = DeviceBuffer((N,), np.int32).poison(); ob = DeviceBuffer((N, cap, 4)).poison(); os_ = DeviceBuffer((N, cap)).poison(); ol = DeviceBuffer((N, cap), np.int32).poison()
    a = RetinaPostArgs(N, 1, pool.cap, ncls, det_per_img, cap, nms_flags, nms_thr, pool.boxes.ptr, pool.scores.ptr, pool.labels.ptr, pool.cnt.ptr, ws.ptr, wsb,
                       oc.ptr, ob.ptr, os_.ptr, ol.ptr)
    check(lib().isegmi_op_retina_postprocess(C.byref(a), None))
    c = oc.numpy(); B = ob.numpy(); S = os_.numpy(); Lb = ol.numpy()
    return [(B[i, : c[i]], S[i, : c[i]], Lb[i, : c[i]]) for i in range(N)]


# ---------------------------------------------------------------- YOLOv3 tail and route
def yolo_slice_records(Cc):
    """Anchor records one block of yolo_select's first launch takes for class count Cc."""
    return lib().isegmi_op_yolo_slice_records(int(Cc))


def yolo_select_device(heads, strides, anchors_wh, A, top_n, conf_thresh, multi_label, min_wh, canvas_w, canvas_h):
    """isegmi_op_yolo_select on poisoned outputs; heads[l] [N,H_l,W_l,A*(5+C)].  -> the device buffers (boxes, scores, labels, cnt, total), still on the
    device (the chained test hands them to retina_postprocess), and their shapes' N, nl."""
    nl = len(heads)
    hs = [np.ascontiguousarray(x, np.float32) for x in heads]
    N = hs[0].shape[0]
    Cc = hs[0].shape[3] // A - 5
    keep = [DeviceBuffer.from_numpy(x) for x in hs]
    ptrs = (C.c_void_p * nl)(*[b.ptr.value for b in keep])
    grid = (C.c_int32 * (2 * nl))(*[v for x in hs for v in x.shape[1:3]])
    st = (C.c_int32 * nl)(*[int(s) for s in strides])
    an = np.ascontiguousarray(anchors_wh, np.float32).reshape(nl, A, 2)
    wsb = lib().isegmi_op_yolo_select_workspace(nl, N, grid, A, Cc, top_n)
    if wsb < 0:
        raise IsegmiError("isegmi_op_yolo_select_workspace: bad sizes")
    ws = DeviceBuffer((wsb,), np.uint8).poison()
    ob = DeviceBuffer((N, nl * top_n, 4)).poison(); os_ = DeviceBuffer((N, nl * top_n)).poison(); ol = DeviceBuffer((N, nl * top_n), np.int32).poison()
    oc = DeviceBuffer((N, nl), np.int32).poison(); ot = DeviceBuffer((N, nl), np.int32).poison()
    check(lib().isegmi_op_yolo_select(nl, N, ptrs, grid, st, an.ctypes.data_as(C.c_void_p), A, Cc, top_n, conf_thresh, int(multi_label), min_wh, int(canvas_w),
                                      int(canvas_h), ws.ptr, wsb, ob.ptr, os_.ptr, ol.ptr, oc.ptr, ot.ptr, None))
    sync()
    return ob, os_, ol, oc, ot


def yolo_select(heads, strides, anchors_wh, A=3, top_n=1024, conf_thresh=0.5, multi_label=1, min_wh=0.0, canvas_w=416, canvas_h=416):
    """-> (dec, total): dec[l][i] = (boxes, scores, labels) of level l, image i in selection order; total [N, nl] candidates before the cut."""
    nl, N = len(heads), np.asarray(heads[0]).shape[0]
    ob, os_, ol, oc, ot = yolo_select_device(heads, strides, anchors_wh, A, top_n, conf_thresh, multi_label, min_wh, canvas_w, canvas_h)
    c = oc.numpy(); B = ob.numpy().reshape(N, nl, top_n, 4); S = os_.numpy().reshape(N, nl, top_n); Lb = ol.numpy().reshape(N, nl, top_n)
    past = np.arange(top_n)[None, None, :] >= c[:, :, None]   # the rows past a count are filled: zero box, score -1, label 0
    assert (S[past] == -1).all() and (Lb[past] == 0).all() and not B[past].any()
    return [[(B[i, l, : c[i, l]], S[i, l, : c[i, l]], Lb[i, l, : c[i, l]]) for i in range(N)] for l in range(nl)], ot.numpy()


def concat_up2x(coarse, skip):
    """isegmi_op_concat_up2x: coarse [N,Hc,Wc,Cc], skip [N,2Hc,2Wc,Cs] -> [N,2Hc,2Wc,Cc+Cs]."""
    coarse = np.ascontiguousarray(coarse, np.float32); skip = np.ascontiguousarray(skip, np.float32)
    N, Hc, Wc, Cc = coarse.shape
    assert skip.shape[:3] == (N, 2 * Hc, 2 * Wc)
    dc = DeviceBuffer.from_numpy(coarse); ds = DeviceBuffer.from_numpy(skip)
    out = DeviceBuffer((N, 2 * Hc, 2 * Wc, Cc + skip.shape[3])).poison()
    check(lib().isegmi_op_concat_up2x(dc.ptr, N, Hc, Wc, Cc, ds.ptr, skip.shape[3], out.ptr, None))
    return out.numpy()


def maxpool_darknet(x, size, stride, zero_pad=0):
    """isegmi_op_maxpool_darknet: x [N,H,W,C] -> [N,(H-1)//stride+1,(W-1)//stride+1,C]; zero_pad 0: taps outside the map are skipped, 1: they are 0."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x)
    out = DeviceBuffer((N, (H - 1) // max(int(stride), 1) + 1, (W - 1) // max(int(stride), 1) + 1, Cc)).poison()
    check(lib().isegmi_op_maxpool_darknet(dx.ptr, N, H, W, Cc, int(size), int(stride), int(zero_pad), out.ptr, None))
    return out.numpy()


def spp_concat(x, zero_pad=0):
    """isegmi_op_spp_concat: x [N,H,W,C] -> [N,H,W,4C] = [mp13 | mp9 | mp5 | x]."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, Cc = x.shape
    dx = DeviceBuffer.from_numpy(x)
    out = DeviceBuffer((N, H, W, 4 * Cc)).poison()
    check(lib().isegmi_op_spp_concat(dx.ptr, N, H, W, Cc, int(zero_pad), out.ptr, None))
    return out.numpy()


# ---------------------------------------------------------------- fp16 conv (configs[4])
def pack_conv_weights_f16(desc, w_krsc):
    w = np.ascontiguousarray(w_krsc, np.float32)
    n = C.c_int64()
    check(lib().isegmi_conv_packed_halfs(C.byref(desc), C.byref(n)))
    out = np.empty(n.value, np.uint16)
    check(lib().isegmi_pack_conv_weights_f16(C.byref(desc), w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out.view(np.float16)


def stem_f16(x_nhwc3, w_krs4, scale=None, shift=None, tile=0):
    """fp16 stem: fp32 NHWC C=3 batch -> (haloed fp16 image) -> 7x7/2 conv + scale/shift + ReLU, fp16 out."""
    x = np.ascontiguousarray(x_nhwc3, np.float32)
    N, H, W, _ = x.shape
    Cout = w_krs4.shape[0]
    d = make_conv_desc(N, H, W, 4, Cout, 7, 7, 2, 3, 1, tile)
    dx = DeviceBuffer.from_numpy(x); dh = DeviceBuffer((N, H + 6, (W + 7) & ~1, 4), np.float16)
    check(lib().isegmi_op_pad_c3_to_f16_halo(dx.ptr, N, H, W, dh.ptr, None))
    dw = DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w_krs4))
    ds = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dsh = None if shift is None else DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    do = DeviceBuffer((N, ho, wo, Cout), np.float16)
    check(lib().isegmi_op_conv2d_f16(C.byref(d), dh.ptr, dw.ptr, _ptr(ds), _ptr(dsh), None, do.ptr, 0, None))
    return do.numpy(), dh.numpy()


def conv1x1_up2x_add_f16(x, w, scale, shift, coarse):
    """isegmi_op_conv1x1_up2x_add_f16: x fp16 NHWC, w [Cout,1,1,Cin], coarse fp16 [N,Hc,Wc,Cout] -> fp16 [N,H,W,Cout]."""
    x = np.ascontiguousarray(x, np.float16); coarse = np.ascontiguousarray(coarse, np.float16)
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    d = make_conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0, 0, 0)
    dx = DeviceBuffer.from_numpy(x); dw = DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w)); dc = DeviceBuffer.from_numpy(coarse)
    ds = DeviceBuffer.from_numpy(np.asarray(scale, np.float32)); dsh = DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    do = DeviceBuffer((N, H, W, Cout), np.float16)
    check(lib().isegmi_op_conv1x1_up2x_add_f16(C.byref(d), dx.ptr, dw.ptr, ds.ptr, dsh.ptr, dc.ptr, coarse.shape[1], coarse.shape[2], do.ptr, None))
    return do.numpy()


def conv3x3_head_f16(x, w, scale, shift, w2, scale2, shift2):
    """isegmi_op_conv3x3_head_f16: x fp16 NHWC [N,H,W,Cin]; w [256,3,3,Cin]; w2 [cout2,1,1,256].  Returns (fp32 [N,H,W,cout2] or None, fused flag)."""
    x = np.ascontiguousarray(x, np.float16)
    N, H, W, Cin = x.shape
    cout2 = w2.shape[0]
    d = make_conv_desc(N, H, W, Cin, 256, 3, 3, 1, 1, 1, 0)
    d2 = make_conv_desc(N, H, W, 256, cout2, 1, 1, 1, 0, 0, 0)
    dx = DeviceBuffer.from_numpy(x); dw = DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w)); dw2 = DeviceBuffer.from_numpy(pack_conv_weights_f16(d2, w2))
    bufs = [DeviceBuffer.from_numpy(np.asarray(a, np.float32)) for a in (scale, shift, scale2, shift2)]
    do = DeviceBuffer((N, H, W, cout2), np.float32)
    fused = C.c_int(0)
    check(lib().isegmi_op_conv3x3_head_f16(C.byref(d), dx.ptr, dw.ptr, bufs[0].ptr, bufs[1].ptr, dw2.ptr, bufs[2].ptr, bufs[3].ptr, cout2, do.ptr, C.byref(fused), None))
    return (do.numpy() if fused.value else None), bool(fused.value)


def stem_pool_f16(x_nhwc3, w_krs4, scale, shift, flags=0):
    """The fp16 stem in one launch (isegmi_op_stem_pool_f16): fp32 NHWC C=3 batch -> haloed fp16 image -> conv 7x7/2 + BN + ReLU + max-pool 3x3/2, fp16 out."""
    x = np.ascontiguousarray(x_nhwc3, np.float32)
    N, H, W, _ = x.shape
    Cout = w_krs4.shape[0]
    d = make_conv_desc(N, H, W, 4, Cout, 7, 7, 2, 3, 1, 0)
    dx = DeviceBuffer.from_numpy(x); dh = DeviceBuffer((N, H + 6, (W + 7) & ~1, 4), np.float16)
    check(lib().isegmi_op_pad_c3_to_f16_halo(dx.ptr, N, H, W, dh.ptr, None))
    dw = DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w_krs4))
    ds = DeviceBuffer.from_numpy(np.asarray(scale, np.float32)); dsh = DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    do = DeviceBuffer((N, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, Cout), np.float16)
    check(lib().isegmi_op_stem_pool_f16(N, H, W, dh.ptr, dw.ptr, ds.ptr, dsh.ptr, do.ptr, int(flags), None))
    return do.numpy()


def conv2d_f16(x, w_krsc, stride=1, pad=0, scale=None, shift=None, residual=None, act=0, tile=0, out_f32=False, out_shape=None, out_div=0,
               out_img_stride=0, out_pix_stride=0, out_offset=0):
    """x fp16-representable NHWC (any float dtype; cast to fp16), returns fp16 (or fp32 when out_f32) as numpy.  out_shape / out_div / out_img_stride /
    out_pix_stride / out_offset: the strided output mode, as conv2d (strides and offset in elements of the output type)."""
    x = np.ascontiguousarray(x, np.float16)
    N, H, W, Cin = x.shape
    Cout, R, S, _ = w_krsc.shape
    d = make_conv_desc(N, H, W, Cin, Cout, R, S, stride, pad, act, tile, out_div, out_img_stride, out_pix_stride)
    ho, wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    dx = DeviceBuffer.from_numpy(x); dw = DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w_krsc))
    ds = None if scale is None else DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dh = None if shift is None else DeviceBuffer.from_numpy(np.asarray(shift, np.float32))
    dr = None if residual is None else DeviceBuffer.from_numpy(np.ascontiguousarray(residual, np.float16))
    do, first = _strided_out((N, ho, wo, Cout), np.float32 if out_f32 else np.float16, out_shape, out_offset)
    check(lib().isegmi_op_conv2d_f16(C.byref(d), dx.ptr, dw.ptr, _ptr(ds), _ptr(dh), _ptr(dr), first, int(out_f32), None))
    return do.numpy()


def bottleneck_ds_f16(x, w1, sb1, w2, sb2, w3, sb3, wd, sbd, flags=0):
    """First block of res2 with its projection shortcut (isegmi_op_bottleneck_ds_f16): x fp16 [N,H,W,64]; wd [256,1,1,64].  Returns fp16 [N,H,W,256]."""
    x = np.ascontiguousarray(x, np.float16)
    N, H, W, Cin = x.shape
    Cmid = w1.shape[0]
    bufs = []
    for w, (sc, sh) in ((w1, sb1), (w2, sb2), (w3, sb3), (wd, sbd)):
        Cout, R, S, Ci = w.shape
        d = make_conv_desc(N, H, W, Ci, Cout, R, S, 1, R // 2, 1, 0)
        bufs += [DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w)), DeviceBuffer.from_numpy(np.asarray(sc, np.float32)),
                 DeviceBuffer.from_numpy(np.asarray(sh, np.float32))]
    dx = DeviceBuffer.from_numpy(x)
    do = DeviceBuffer((N, H, W, 4 * Cmid), np.float16)
    bd = BottleneckDesc(N, H, W, Cin, Cmid, int(flags))
    check(lib().isegmi_op_bottleneck_ds_f16(C.byref(bd), dx.ptr, *[b.ptr for b in bufs], do.ptr, None))
    return do.numpy()


def bottleneck_f16(x, w1, sb1, w2, sb2, w3, sb3, flags=0):
    """Fused identity bottleneck (isegmi_op_bottleneck_f16): x fp16 NHWC [N,H,W,Cin]; w1 [Cmid,1,1,Cin], w2 [Cmid,3,3,Cmid],
    w3 [Cin,1,1,Cmid] natural KRSC fp32 (rounded to fp16 by the packer); sb* = (scale, shift) of the folded BN.  Returns fp16 numpy."""
    x = np.ascontiguousarray(x, np.float16)
    N, H, W, Cin = x.shape
    Cmid = w1.shape[0]
    bufs = []
    for w, (sc, sh) in ((w1, sb1), (w2, sb2), (w3, sb3)):
        Cout, R, S, Ci = w.shape
        d = make_conv_desc(N, H, W, Ci, Cout, R, S, 1, R // 2, 1, 0)
        bufs += [DeviceBuffer.from_numpy(pack_conv_weights_f16(d, w)), DeviceBuffer.from_numpy(np.asarray(sc, np.float32)),
                 DeviceBuffer.from_numpy(np.asarray(sh, np.float32))]
    dx = DeviceBuffer.from_numpy(x)
    do = DeviceBuffer((N, H, W, Cin), np.float16)
    bd = BottleneckDesc(N, H, W, Cin, Cmid, int(flags))
    check(lib().isegmi_op_bottleneck_f16(C.byref(bd), dx.ptr, *[b.ptr for b in bufs], do.ptr, None))
    return do.numpy()


# ---------------------------------------------------------------- COCO RLE on the device
def rle_encode(masks, count=None, image_hw=None, cap_runs=None, cap_chars=None, windows=None):
    """masks [N,K,h,w] uint8 -> (run_off [N*K+1], counts, str_off [N*K+1], chars bytes, status [4]): pycocotools rleEncode + rleToString of
    every valid slot (k < count[n]) over the top-left image_hw[n] window of its plane (host convenience wrapper of isegmi_op_rle_encode).
    windows [N, K, 4] (x0, y0, x1, y1): every set pixel of a slot lies inside its window; nothing outside it is read."""
    masks = np.ascontiguousarray(masks, np.uint8)
    N, K, h, w = masks.shape
    cap_runs = int(cap_runs or max(1024, -(-(masks.size + N * K) // 1024) * 1024))  # worst case: every pixel starts a run
    cap_chars = int(cap_chars or 7 * cap_runs)
    sz = [C.c_int64() for _ in range(6)]
    check(lib().isegmi_rle_workspace(N, K, h, w, cap_runs, *[C.byref(s) for s in sz]))
    ws = [DeviceBuffer((s.value,), np.uint8) for s in sz]
    dm = DeviceBuffer.from_numpy(masks)
    dc = None if count is None else DeviceBuffer.from_numpy(np.ascontiguousarray(count, np.int32))
    dh = None if image_hw is None else DeviceBuffer.from_numpy(np.ascontiguousarray(image_hw, np.int32).reshape(N, 2))
    dwin = None if windows is None else DeviceBuffer.from_numpy(np.ascontiguousarray(windows, np.int32).reshape(N, K, 4))
    ro = DeviceBuffer((N * K + 1,), np.int32); cn = DeviceBuffer((cap_runs,), np.uint32); so = DeviceBuffer((N * K + 1,), np.int32)
    ch = DeviceBuffer((cap_chars,), np.uint8); stt = DeviceBuffer((4,), np.int32)
    a = RleArgs(N, K, h, w, cap_runs, cap_chars, dm.ptr, _ptr(dc), _ptr(dh), _ptr(dwin), ws[0].ptr, ws[1].ptr, ws[2].ptr, ws[3].ptr, ws[4].ptr, ws[5].ptr,
                ro.ptr, cn.ptr, so.ptr, ch.ptr, stt.ptr)
    check(lib().isegmi_op_rle_encode(C.byref(a), None))
    sync()
    return ro.numpy(), cn.numpy(), so.numpy(), ch.numpy().tobytes(), stt.numpy()


# ---------------------------------------------------------------- Pose2Seg pose-guided stages (csrc/pose2seg_ops.hip)
def p2s_letterbox(d_u8, d_table, N, S, mean3, std3, swap_rb, round_u8, d_out, stream=None):
    m = (C.c_float * 3)(*[float(v) for v in mean3]); sd = (C.c_float * 3)(*[float(v) for v in std3])
    check(lib().isegmi_op_pose2seg_letterbox(_ptr(d_u8), _ptr(d_table), int(N), int(S), m, sd, int(bool(swap_rb)), int(bool(round_u8)), _ptr(d_out),
                                             stream))


def p2s_fit(d_kpts, d_roi_img, R, d_m1, d_templates, T, align_corners, d_m3, d_G, d_mmask, d_kalign, d_fit, stream=None):
    check(lib().isegmi_op_pose2seg_fit(_ptr(d_kpts), _ptr(d_roi_img), int(R), _ptr(d_m1), _ptr(d_templates), int(T), int(bool(align_corners)),
                                       _ptr(d_m3), _ptr(d_G), _ptr(d_mmask), _ptr(d_kalign), _ptr(d_fit), stream))


def p2s_align(d_feat, Hf, Wf, Cc, d_roi_img, d_G, R, d_out, out_c, stream=None):
    check(lib().isegmi_op_pose2seg_align(_ptr(d_feat), int(Hf), int(Wf), int(Cc), _ptr(d_roi_img), _ptr(d_G), int(R), _ptr(d_out), int(out_c), stream))


def p2s_skeleton(d_kalign, R, d_out, out_c, c0, stream=None):
    check(lib().isegmi_op_pose2seg_skeleton(_ptr(d_kalign), int(R), _ptr(d_out), int(out_c), int(c0), stream))


def p2s_masks(d_logits, d_mmask, d_counts, d_roi_off, d_image_hw, N, K, Hmax, Wmax, d_ws_box, d_masks, d_boxes, d_scores, d_labels, d_count_out,
              stream=None):
    check(lib().isegmi_op_pose2seg_masks(_ptr(d_logits), _ptr(d_mmask), _ptr(d_counts), _ptr(d_roi_off), _ptr(d_image_hw), int(N), int(K),
                                         int(Hmax), int(Wmax), _ptr(d_ws_box), _ptr(d_masks), _ptr(d_boxes), _ptr(d_scores), _ptr(d_labels),
                                         _ptr(d_count_out), stream))


def pose_handoff(score, count, kpt, kscore, ratios_wh, person_thresh, kp_thresh, K, poison=True):
    """isegmi_op_pose_handoff on host arrays (tests, diagnostics): score [N, cap], count [N], kpt [N, cap, NK, 3], kscore [N, cap, NK], ratios_wh [N, 2] ->
    (kpts_out [N * K, 17, 3] -- the first count_out.sum() rows are the persons --, score_out [N, K], src_slot [N, K], count_out [N]).  The outputs start
    out as 0xFF bytes (`poison`), so a slot the kernel did not write shows."""
    score = np.ascontiguousarray(score, np.float32)
    N, cap = score.shape
    kpt = np.ascontiguousarray(kpt, np.float32)
    NK = kpt.shape[2]
    ins = [DeviceBuffer.from_numpy(a) for a in (score, np.ascontiguousarray(count, np.int32), kpt, np.ascontiguousarray(kscore, np.float32),
                                                np.ascontiguousarray(ratios_wh, np.float32))]
    outs = [DeviceBuffer((N * K, 17, 3)), DeviceBuffer((N, K)), DeviceBuffer((N, K), np.int32), DeviceBuffer((N,), np.int32)]
    if poison:
        for o in outs:
            o.poison()
    check(lib().isegmi_op_pose_handoff(*[b.ptr for b in ins], int(N), int(cap), int(NK), float(person_thresh), float(kp_thresh), int(K),
                                       *[b.ptr for b in outs], None))
    sync()
    return tuple(o.numpy() for o in outs)


# ---------------------------------------------------------------- COCO evaluation on the device (csrc/cocoeval.hip)
class RleSet:
    """M run-length encodings on the device, prefix-summed once (isegmi_op_rle_prefix): the operand of rle_iou.
    counts_list: per RLE its run counts (column-major, zeros first, as isegmi.coco.rle_from_string yields them); hw [M][2] = (h, w).
    .area [M] int64 and .bbox [M][4] int32 (x0, y0, x1, y1 inclusive; (0, 0, -1, -1) when empty) are downloaded on first use."""

    def __init__(self, counts_list, hw, stream=None):
        self.M = len(counts_list)
        hw = np.ascontiguousarray(hw, np.int32).reshape(self.M, 2)
        lens = np.fromiter((len(c) for c in counts_list), np.int64, self.M)
        off = np.zeros(self.M + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        total = int(off[-1])
        flat = np.concatenate([np.asarray(c, np.int64).ravel() for c in counts_list]) if total else np.zeros(0, np.int64)
        if total and (flat.min() < 0 or flat.max() >= 1 << 32):
            raise IsegmiError("RLE run counts must fit uint32")
        sz = [C.c_int64() for _ in range(4)]
        check(lib().isegmi_coco_rle_prefix_bytes(total, self.M, *[C.byref(s) for s in sz]))
        self.d_counts = DeviceBuffer.from_numpy(flat.astype(np.uint32))
        self.d_off = DeviceBuffer.from_numpy(off)
        self.d_hw = DeviceBuffer.from_numpy(hw)
        self.d_bounds = DeviceBuffer((sz[0].value // 4,), np.uint32)
        self.d_cum = DeviceBuffer((sz[1].value // 4,), np.uint32)
        self.d_area = DeviceBuffer((sz[2].value // 8,), np.int64)
        self.d_bbox = DeviceBuffer((sz[3].value // 16, 4), np.int32)
        self.off, self.hw, self.total_runs = off, hw, total
        self._area = self._bbox = None
        import time
        sync()
        t0 = time.perf_counter()
        self.prefix(stream)
        sync()
        self.prefix_seconds = time.perf_counter() - t0      # the prefix kernel alone, uploads excluded (tools/cocoeval_bench.py)

    def prefix(self, stream=None):
        check(lib().isegmi_op_rle_prefix(self.d_counts.ptr, self.d_off.ptr, self.d_hw.ptr, self.M, self.d_bounds.ptr, self.d_cum.ptr,
                                              self.d_area.ptr, self.d_bbox.ptr, stream))

    @property
    def area(self):
        if self._area is None:
            sync()
            self._area = self.d_area.numpy()
        return self._area

    @property
    def bbox(self):
        if self._bbox is None:
            sync()
            self._bbox = self.d_bbox.numpy()
        return self._bbox

    def free(self):
        for b in (self.d_counts, self.d_off, self.d_hw, self.d_bounds, self.d_cum, self.d_area, self.d_bbox):
            b.free()


def rle_iou_device(rles, d_pairs, P, d_out, stream=None):
    """isegmi_op_rle_iou over device buffers: d_pairs [P][3] int32 (det, gt, crowd) -> d_out [P] float64."""
    check(lib().isegmi_op_rle_iou(rles.d_bounds.ptr, rles.d_cum.ptr, rles.d_off.ptr, rles.d_hw.ptr, rles.d_area.ptr, rles.d_bbox.ptr,
                                       rles.M, _ptr(d_pairs), int(P), _ptr(d_out), stream))


def rle_iou(rles, pairs):
    """Host convenience: pairs [P][3] (det RLE, gt RLE, crowd) of an RleSet -> float64 [P]."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 3)
    dp = DeviceBuffer.from_numpy(pairs); do = DeviceBuffer((len(pairs),), np.float64)
    rle_iou_device(rles, dp, len(pairs), do)
    sync()
    out = do.numpy()
    dp.free(); do.free()
    return out


def bbox_iou_device(d_boxes, B, d_pairs, P, d_out, stream=None):
    check(lib().isegmi_op_bbox_iou(_ptr(d_boxes), int(B), _ptr(d_pairs), int(P), _ptr(d_out), stream))


def bbox_iou(boxes, pairs):
    """Host convenience: boxes [B][4] float64 xywh, pairs [P][3] (det box, gt box, crowd) -> float64 [P] in bbIou's operation order."""
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 3)
    db = DeviceBuffer.from_numpy(boxes); dp = DeviceBuffer.from_numpy(pairs); do = DeviceBuffer((len(pairs),), np.float64)
    bbox_iou_device(db, len(boxes), dp, len(pairs), do)
    sync()
    out = do.numpy()
    for b in (db, dp, do):
        b.free()
    return out


def oks_device(d_kpts, d_box, d_area, d_vars, M, K, d_pairs, P, d_out, stream=None):
    """isegmi_op_oks over device buffers: d_kpts [M][K][3], d_box [M][4], d_area [M], d_vars [K] float64; d_pairs [P][3] int32 -> d_out [P] float64."""
    check(lib().isegmi_op_oks(_ptr(d_kpts), _ptr(d_box), _ptr(d_area), _ptr(d_vars), int(M), int(K), _ptr(d_pairs), int(P), _ptr(d_out),
                                   stream))


def oks(kpts, box, area, variances, pairs):
    """Host convenience: kpts [M][K][3] (x, y, v), box [M][4] xywh, area [M], variances [K] = (sigmas * 2) ** 2, pairs [P][3] (det item, gt item,
    unused) -> float64 [P] in computeOks' operation order, the terms added in keypoint-index order."""
    variances = np.ascontiguousarray(variances, np.float64).ravel()
    K = len(variances)
    kpts = np.ascontiguousarray(kpts, np.float64).reshape(-1, K, 3)
    M = len(kpts)
    box = np.ascontiguousarray(box, np.float64).reshape(M, 4); area = np.ascontiguousarray(area, np.float64).reshape(M)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 3)
    bufs = [DeviceBuffer.from_numpy(a) for a in (kpts, box, area, variances, pairs)]
    do = DeviceBuffer((len(pairs),), np.float64)
    oks_device(*bufs[:4], M, K, bufs[4], len(pairs), do)
    sync()
    out = do.numpy()
    for b in bufs + [do]:
        b.free()
    return out


def coco_match(det_off, gt_off, iou_off, ious, det_area, gt_area, gt_crowd, gt_ignore, area_rng, iou_thrs, d_ious=None, stream=None):
    """isegmi_op_coco_match: -> (dt_match [A,T,n_dets] int32, dt_ignore [A,T,n_dets] uint8, gt_match [A,T,n_gts] int32, gt_ignore [A,n_gts] uint8).
    ious: host float64 array, or None with d_ious = a DeviceBuffer that already holds the blocks (the output of rle_iou_device)."""
    det_off = np.ascontiguousarray(det_off, np.int64); gt_off = np.ascontiguousarray(gt_off, np.int64)
    iou_off = np.ascontiguousarray(iou_off, np.int64)
    n_groups = len(iou_off)
    assert len(det_off) == n_groups + 1 and len(gt_off) == n_groups + 1
    area_rng = np.ascontiguousarray(area_rng, np.float64).reshape(-1, 2); iou_thrs = np.ascontiguousarray(iou_thrs, np.float64).ravel()
    A, T = len(area_rng), len(iou_thrs)
    n_dets, n_gts = int(det_off[-1]) if n_groups else 0, int(gt_off[-1]) if n_groups else 0
    own = []

    def up(a, dt):
        b = DeviceBuffer.from_numpy(np.ascontiguousarray(a, dt))
        own.append(b)
        return b
    if d_ious is None:
        d_ious = up(np.asarray(ious, np.float64).ravel(), np.float64)
    n_ious = d_ious.nbytes // 8
    sz = [C.c_int64() for _ in range(4)]
    check(lib().isegmi_coco_match_bytes(n_dets, n_gts, A, T, *[C.byref(s) for s in sz]))
    o_dtm = DeviceBuffer((A, T, n_dets), np.int32); o_dti = DeviceBuffer((A, T, n_dets), np.uint8)
    o_gtm = DeviceBuffer((A, T, n_gts), np.int32); o_gti = DeviceBuffer((A, n_gts), np.uint8)
    own += [o_dtm, o_dti, o_gtm, o_gti]
    assert [o_dtm.nbytes, o_dti.nbytes, o_gtm.nbytes, o_gti.nbytes] == [s.value for s in sz]
    for b in (o_dtm, o_dti, o_gtm, o_gti):
        if b.nbytes:
            b.zero()
    a = CocoMatchArgs(n_groups, A, T, 0, n_dets, n_gts, n_ious, up(det_off, np.int64).ptr, up(gt_off, np.int64).ptr, up(iou_off, np.int64).ptr,
                      d_ious.ptr, up(det_area, np.float64).ptr, up(gt_area, np.float64).ptr, up(gt_crowd, np.uint8).ptr,
                      up(gt_ignore, np.uint8).ptr, up(area_rng, np.float64).ptr, up(iou_thrs, np.float64).ptr,
                      o_dtm.ptr, o_dti.ptr, o_gtm.ptr, o_gti.ptr)
    check(lib().isegmi_op_coco_match(C.byref(a), stream))
    sync()
    out = (o_dtm.numpy(), o_dti.numpy(), o_gtm.numpy(), o_gti.numpy())
    for b in own:
        b.free()
    return out


# ---- ViT operators (csrc/vit_ops.hip) on host arrays: tests and small inputs
def attention(qkv, heads, pad_floats=0, pad_value=0.0):
    """isegmi_op_attention of qkv [N, T, 3 * heads * 64] -> [N, T, heads * 64].  pad_floats: the device buffer is that much longer than the tensor and
    the excess holds pad_value (a kernel that read past the last token would pick it up)."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    N, T, C3 = qkv.shape
    assert C3 == 3 * heads * 64, (qkv.shape, heads)
    flat = np.concatenate([qkv.reshape(-1), np.full(int(pad_floats), pad_value, np.float32)])
    dq = DeviceBuffer.from_numpy(flat); do = DeviceBuffer((N, T, heads * 64)).poison()
    check(lib().isegmi_op_attention(dq.ptr, N, T, heads, do.ptr, None))
    return do.numpy()


def layer_norm(x, gamma, beta, eps=1e-6, inplace=False, rows=None, x_row_stride=None, out_row_stride=None):
    """isegmi_op_layer_norm of x [..., D].  rows / x_row_stride: only `rows` rows, x_row_stride floats apart, are normalised -> [rows, D] (the class-token
    form).  out_row_stride (with rows): the output rows are that many floats apart in a poisoned buffer -> the whole buffer [rows, out_row_stride], gaps
    included.  D is gamma's length.  In place with rows: x is [rows, x_row_stride], out_row_stride is x_row_stride -> the whole buffer after the call."""
    x = np.ascontiguousarray(x, np.float32)
    dg = DeviceBuffer.from_numpy(np.ascontiguousarray(gamma, np.float32)); db = DeviceBuffer.from_numpy(np.ascontiguousarray(beta, np.float32))
    D = dg.shape[0]
    dx = DeviceBuffer.from_numpy(x)
    assert dg.shape == (D,) and db.shape == (D,), (dg.shape, db.shape, D)
    if rows is None:
        assert x.shape[-1] == D and out_row_stride is None
        do = dx if inplace else DeviceBuffer(x.shape).poison()
        check(lib().isegmi_op_layer_norm(dx.ptr, x.size // D, D, D, dg.ptr, db.ptr, float(eps), do.ptr, D, None))
        return do.numpy()
    xs = int(x_row_stride)
    os_ = xs if inplace and out_row_stride is None else D if out_row_stride is None else int(out_row_stride)
    assert rows == 0 or (rows - 1) * xs + D <= x.size
    if inplace:
        assert os_ == xs, (os_, xs)
        do = dx
    else:
        do = DeviceBuffer((rows, max(os_, D))).poison()
    check(lib().isegmi_op_layer_norm(dx.ptr, rows, D, xs, dg.ptr, db.ptr, float(eps), do.ptr, os_, None))
    return do.numpy()


def gelu(x, gelu_tanh=False, inplace=False):
    x = np.ascontiguousarray(x, np.float32)
    dx = DeviceBuffer.from_numpy(x)
    dy = dx if inplace else DeviceBuffer(x.shape).poison()
    check(lib().isegmi_op_gelu(dx.ptr, dy.ptr, x.size, 1 if gelu_tanh else 0, None))
    return dy.numpy()


def patchify(x_nhwc3, P):
    x = np.ascontiguousarray(x_nhwc3, np.float32)
    N, H, W, c = x.shape
    assert c == 3
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer((N, H // P, W // P, P * P * 3)).poison()
    check(lib().isegmi_op_patchify(dx.ptr, N, H, W, P, do.ptr, None))
    return do.numpy()


def class_softmax(logits):
    x = np.ascontiguousarray(logits, np.float32)
    rows, n = x.shape
    dx = DeviceBuffer.from_numpy(x); do = DeviceBuffer(x.shape).poison()
    check(lib().isegmi_op_class_softmax(dx.ptr, rows, n, do.ptr, None))
    return do.numpy()


# ---- the painter (csrc/render.hip) on host arrays: tests and tools
def paint_lists(entries, dots):
    """-> (entries int32 [D, 8], dots int32 [Q, 4]) as isegmi_op_paint / isegmi_engine_paint read them; None is an empty list."""
    e = np.zeros((0, 8), np.int32) if entries is None else np.ascontiguousarray(entries, np.int32).reshape(-1, 8)
    d = np.zeros((0, 4), np.int32) if dots is None else np.ascontiguousarray(dots, np.int32).reshape(-1, 4)
    return e, d


def paint(image_u8, masks=None, entries=None, dots=None, inplace=False, tail=0, sentinel=0xA5, offset=0):
    """isegmi_op_paint of image [H, W, 3] uint8 with masks [slots, ph, pw] uint8 (None: no planes).  The output buffer is `tail` bytes longer than the
    image and pre-filled with `sentinel`; `offset` shifts the image, the planes and the output that many bytes into their allocations (unaligned bases).
    -> (rc, out bytes [H * W * 3 + tail], the input buffer's H * W * 3 bytes after the call); rc is returned, not raised: the refusals are results."""
    img = np.ascontiguousarray(image_u8, np.uint8)
    H, W = img.shape[:2]
    n = img.size
    e, d = paint_lists(entries, dots)
    d_in = DeviceBuffer((offset + n + (tail if inplace else 0),), np.uint8)
    d_in.upload(np.concatenate([np.zeros(offset, np.uint8), img.reshape(-1), np.full(tail if inplace else 0, sentinel, np.uint8)]))
    d_out = d_in if inplace else DeviceBuffer((offset + n + tail,), np.uint8)
    if not inplace:
        d_out.upload(np.full(offset + n + tail, sentinel, np.uint8))
    d_m, slots, ph, pw = None, 0, 0, 0
    if masks is not None:
        m = np.ascontiguousarray(masks, np.uint8)
        slots, ph, pw = m.shape
        d_m = DeviceBuffer.from_numpy(np.concatenate([np.zeros(offset, np.uint8), m.reshape(-1)]))
    d_e = DeviceBuffer.from_numpy(e) if len(e) else None
    d_d = DeviceBuffer.from_numpy(d) if len(d) else None
    at = lambda b: None if b is None else C.c_void_p(b.ptr.value + offset)   # noqa: E731
    rc = lib().isegmi_op_paint(at(d_in), H, W, at(d_m), slots, ph, pw, _ptr(d_e), len(e), _ptr(d_d), len(d), at(d_out), None)
    check(lib().isegmi_sync())
    out, src = d_out.numpy()[offset:], d_in.numpy()[offset:offset + n]
    for b in {id(x): x for x in (d_in, d_out, d_m, d_e, d_d) if x is not None}.values():
        b.free()
    return rc, out, src
