"""The model-independent half of an engine wrapper: one `isegmi_engine` handle and everything every model does with it -- parameters, weight
marshalling, streams and marks, named buffers, the uint8 front end, the device-side COCO output and the asynchronous download slots.
Yolact, MaskRCNN (and with it RetinaNet), Pose2Seg and YoloV3 derive from Engine; isegmi.pipeline and isegmi.dist drive this interface."""
import ctypes as C

import numpy as np

from . import _ffi

_DTYPES = (np.float32, np.int32, np.uint8, np.int64, np.float16)   # isegmi_engine_buffer_info's dtype codes


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _addr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Engine:
    KIND = None   # model_kind of isegmi_engine_create
    _h = None     # the handle (bench.py and the tools read it)

    def _create(self, device, max_batch, H, W):
        """isegmi_engine_create(KIND, max_batch, H, W) on `device`.  A subclass calls this once its configuration refusals are through."""
        _ffi.set_device(device)
        self._h = C.c_void_p()
        _ffi.check(_ffi.lib().isegmi_engine_create(self.KIND, max_batch, H, W, C.byref(self._h)))

    def set_param(self, name, value):
        _ffi.check(_ffi.lib().isegmi_engine_set_param(self._h, name.encode(), value))

    def param(self, name, default=None):
        """The value set_param last gave `name` on this engine (read back from the engine, isegmi_engine_get_param), else `default`: the engine's
        own defaults live in the C++ code that reads each parameter, so the caller names the one it means."""
        v, is_set = C.c_float(), C.c_int32()
        _ffi.check(_ffi.lib().isegmi_engine_get_param(self._h, name.encode(), 0.0, C.byref(v), C.byref(is_set)))
        return float(v.value) if is_set.value else default

    # -- weights -------------------------------------------------------------------------------
    def _set_conv_krsc(self, name, w, scale=None, shift=None):
        """One layer, natural [Cout][R][S][Cin] weights with the folded scale / shift [Cout] (None: 1 / 0)."""
        w, sc, sh = _f32(w), _f32(scale), _f32(shift)
        cout, r, s, cin = w.shape
        _ffi.check(_ffi.lib().isegmi_engine_set_conv(self._h, name.encode(), cout, r, s, cin, _addr(w), _addr(sc), _addr(sh)))

    def _set_conv_grouped(self, name, w, groups, scale, shift):
        """A grouped 3x3 layer: w [Cout][3][3][Cout / groups]."""
        w, sc, sh = _f32(w), _f32(scale), _f32(shift)
        _ffi.check(_ffi.lib().isegmi_engine_set_conv_grouped(self._h, name.encode(), w.shape[0], groups, _addr(w), _addr(sc), _addr(sh)))

    def _set_tensor(self, name, a):
        a = np.ascontiguousarray(a)
        _ffi.check(_ffi.lib().isegmi_engine_set_tensor(self._h, name.encode(), _addr(a), a.nbytes))

    # -- streams, marks, timings -----------------------------------------------------------------
    def sync(self):
        _ffi.check(_ffi.lib().isegmi_engine_sync(self._h))

    def stream(self):
        """the stream the last forward's results (and everything packed or handed off from them) complete on"""
        st = C.c_void_p()
        _ffi.check(_ffi.lib().isegmi_engine_stream(self._h, C.byref(st)))
        return st

    def mark_step(self):
        _ffi.check(_ffi.lib().isegmi_engine_mark_step(self._h))

    def wait_mark(self, back=0):
        """host wait for the completion mark `back` marks before the newest one: bounds the steps a producer loop keeps in flight"""
        _ffi.check(_ffi.lib().isegmi_engine_wait_mark(self._h, int(back)))

    def step_times(self, cap=65536):
        """Intervals (ms) between consecutive mark_step() completion marks; clears the marks."""
        ms = (C.c_float * cap)(); cnt = C.c_int()
        _ffi.check(_ffi.lib().isegmi_engine_step_times(self._h, ms, cap, C.byref(cnt)))
        return [float(ms[i]) for i in range(cnt.value)]

    def timings(self):
        names = C.create_string_buffer(4096); ms = (C.c_float * 64)(); cnt = C.c_int()
        _ffi.check(_ffi.lib().isegmi_engine_get_timings(self._h, names, 4096, ms, 64, C.byref(cnt)))
        ns = names.value.decode().split(";") if cnt.value else []
        return [(ns[i], float(ms[i])) for i in range(cnt.value)]

    def conv_stats(self):
        """(flops, ms, launches) of the conv launches since the last call (needs set_param("conv_timing", 1))."""
        f, ms, n = C.c_double(), C.c_double(), C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_conv_stats(self._h, C.byref(f), C.byref(ms), C.byref(n)))
        return f.value, ms.value, n.value

    # -- named buffers ---------------------------------------------------------------------------
    def _buffer_info(self, name):
        """-> (device pointer, bytes, numpy dtype, shape) of a named engine buffer"""
        p = C.c_void_p(); nb = C.c_int64(); dt = C.c_int32(); nd = C.c_int32(); shp = (C.c_int64 * 4)()
        _ffi.check(_ffi.lib().isegmi_engine_buffer_info(self._h, name.encode(), C.byref(p), C.byref(nb), C.byref(dt), shp, C.byref(nd)))
        return p, nb.value, _DTYPES[dt.value], tuple(int(shp[i]) for i in range(nd.value))

    def fetch(self, name, rows=None):
        """D2H copy of a named engine buffer (optionally only its first `rows` leading rows)."""
        p, _, dtype, shape = self._buffer_info(name)
        if rows is not None:
            shape = (rows,) + shape[1:]
        out = np.empty(shape, dtype)
        if out.nbytes:
            _ffi.check(_ffi.lib().isegmi_d2h(_addr(out), p, out.nbytes))
        return out

    def memory(self):
        """(weight_bytes, buffer_bytes) of device memory held by the engine (+ the input slots owned by this wrapper)."""
        wb, bb = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_memory(self._h, C.byref(wb), C.byref(bb)))
        extra = sum(b.nbytes for b in (getattr(self, "_d_in", None), getattr(self, "_d_in2", None)) if b is not None)
        return wb.value, bb.value + extra

    # -- input: fp32 batches from pinned memory, uint8 images through the device front end -----------
    def input_buffer(self, slot=0):
        """Device input buffer `slot` (0 or 1; the second one is allocated on first use, for double-buffered uploads)."""
        if slot == 0:
            return self._d_in
        if getattr(self, "_d_in2", None) is None:
            self._d_in2 = _ffi.DeviceBuffer(self._d_in.shape)
        return self._d_in2

    def upload_async(self, pinned, slot=0):
        """Asynchronous H2D of a whole batch from a _ffi.PinnedBuffer into input buffer `slot` on the engine's copy stream; the
        next forward is ordered behind it and it is ordered behind the previous forward's read of its input."""
        d = self.input_buffer(slot)
        assert pinned.nbytes <= d.nbytes
        _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, d.ptr, pinned.ptr, pinned.nbytes))

    def _u8_staging(self, slot, nbytes):
        st = getattr(self, "_u8", None)
        if st is None:
            st = self._u8 = [None, None]
        if st[slot] is None or st[slot].nbytes < nbytes:
            if st[slot] is not None:
                self.sync()  # a queued transform may still read the old buffer
                st[slot].free()
            st[slot] = _ffi.DeviceBuffer((int(nbytes),), np.uint8)
        return st[slot]

    def _preprocess_u8(self, d_u8_ptr, n, hin, win, d_out_ptr, hout, wout, hpad, wpad, mean, std, swap_rb, hflip=False):
        """hflip: the image mirrored within its own width (isegmi_engine_preprocess_u8_flip; the mirrored views of TEST.BBOX_AUG)"""
        m = (C.c_float * 3)(*[float(v) for v in mean]); sd = (C.c_float * 3)(*[float(v) for v in std])
        if hflip:
            return _ffi.check(_ffi.lib().isegmi_engine_preprocess_u8_flip(self._h, C.c_void_p(d_u8_ptr), n, hin, win, C.c_void_p(d_out_ptr), hout, wout, hpad,
                                                                          wpad, hpad * wpad * 3, m, sd, 1 if swap_rb else 0, 1))
        _ffi.check(_ffi.lib().isegmi_engine_preprocess_u8(self._h, C.c_void_p(d_u8_ptr), n, hin, win, C.c_void_p(d_out_ptr), hout, wout, hpad, wpad,
                                                          hpad * wpad * 3, m, sd, 1 if swap_rb else 0))

    def _resample_u8(self, st, plan, view, d_out_ptr, planes, hpad, wpad, mean, std, swap_rb, fill=0.0):
        """isegmi_engine_resample_u8: launch `view` of a transforms.ResamplePlan whose blob sits in staging buffer `st` -> `planes` fp32
        canvases of hpad x wpad at d_out_ptr: PIL-exact resize, normalisation, padding, one launch for the view's images."""
        _, tables = plan.header()
        t = tables[view]
        m = (C.c_float * 3)(*[float(v) for v in mean]); sd = (C.c_float * 3)(*[float(v) for v in std])
        _ffi.check(_ffi.lib().isegmi_engine_resample_u8(self._h, st.ptr, plan.nbytes, plan.table_off[view], _addr(t), t.shape[0], plan.coeff_off,
                                                       plan.coeff_words, plan.src_off, C.c_void_p(d_out_ptr), planes, hpad, wpad, hpad * wpad * 3, m, sd,
                                                       1 if swap_rb else 0, float(fill)))

    # -- device-side COCO output: RLE of the masks, one fixed-size record block per batch, asynchronous download slots --------
    def rle_device(self, image_hw=None):
        """pycocotools RLE (counts + compressed strings) of det.masks of the last postprocess / paste, on the results stream; image_hw
        [n, 2] = every image's own (h, w) inside the mask planes (None: the whole plane)."""
        hw = None if image_hw is None else np.ascontiguousarray(image_hw, np.int32).reshape(-1, 2)
        _ffi.check(_ffi.lib().isegmi_engine_rle(self._h, _addr(hw)))

    def coco_record_bytes(self, n):
        """(total bytes, offset of the strings) of the record block of a batch of n images (isegmi_engine_pack_coco_records)."""
        nb, co = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_coco_record_bytes(self._h, n, C.byref(nb), C.byref(co)))
        return nb.value, co.value

    def pack_coco_records(self, dev_buffer, n_block):
        nb = C.c_int64()
        _ffi.check(_ffi.lib().isegmi_engine_pack_coco_records(self._h, dev_buffer.ptr, dev_buffer.nbytes, int(n_block), C.byref(nb)))
        return nb.value

    def download_async(self, slot, pinned, dev_buffer, nbytes):
        _ffi.check(_ffi.lib().isegmi_engine_download_async(self._h, slot, pinned.ptr, dev_buffer.ptr, nbytes))

    def download_fence(self, slot):
        _ffi.check(_ffi.lib().isegmi_engine_download_fence(self._h, slot))

    def download_wait(self, slot):
        _ffi.check(_ffi.lib().isegmi_engine_download_wait(self._h, slot))

    # -- the painter: the annotated image of a demo, drawn where the masks are ---------------------------------------
    def paint_device(self, image_u8, entries, dots=None, index=0):
        """isegmi_engine_paint: the draw list `entries` (int32 [D, 8], isegmi.render) and `dots` (int32 [Q, 4]) on image [H, W, 3] uint8,
        masks = det.masks of image `index` of the last paste / postprocess.  H * W * 3 bytes go up and come back; the mask planes stay on the device.
        -> the painted image (a new array)."""
        img = np.ascontiguousarray(image_u8, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise TypeError("paint_device takes an HxWx3 uint8 image")
        H, W = img.shape[:2]
        e, d = _ffi.paint_lists(entries, dots)
        buf = getattr(self, "_paint_buf", None)
        if buf is None or buf.nbytes < img.nbytes:
            if buf is not None:
                self.sync()
                buf.free()
            buf = self._paint_buf = _ffi.DeviceBuffer((img.nbytes,), np.uint8)
        _ffi.check(_ffi.lib().isegmi_h2d(buf.ptr, _addr(img), img.nbytes))
        _ffi.check(_ffi.lib().isegmi_engine_paint(self._h, int(index), buf.ptr, H, W, _addr(e) if len(e) else None, len(e),
                                                  _addr(d) if len(d) else None, len(d), buf.ptr))
        self.sync()
        out = np.empty_like(img)
        _ffi.check(_ffi.lib().isegmi_d2h(_addr(out), buf.ptr, out.nbytes))
        return out

    def close(self):
        buf, self._paint_buf = getattr(self, "_paint_buf", None), None
        if buf is not None:
            buf.free()
        if self._h:
            _ffi.lib().isegmi_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DetectionBlock:
    """Mixin of the box detectors (RetinaNet, YoloV3): the four detection buffers of a step as one block through the engine's asynchronous download
    slots (isegmi.predictor.inference).  The class has `cfg.det_cap` and the Engine methods."""
    # -- the four detection buffers of a step through the engine's asynchronous download slots (isegmi.predictor.inference) --------------
    _DET = (("det.count", 4, np.int32), ("det.box", 16, np.float32), ("det.score", 4, np.float32), ("det.label", 4, np.int32))

    def detection_bytes(self, n):
        """Bytes of one step's block for n images: [count i32 x n][box f32 x n*cap*4][score f32 x n*cap][label i32 x n*cap]."""
        K = self.cfg.det_cap
        return sum(n * (b if name == "det.count" else b * K) for name, b, _ in self._DET)

    def download_detections_async(self, slot, pinned, n):
        """Enqueue the copies of the last forward's detection buffers (first n images) into `pinned` behind it; download_wait(slot) then waits for them."""
        K = self.cfg.det_cap
        assert pinned.nbytes >= self.detection_bytes(n)
        off = 0
        for name, b, _ in self._DET:
            nbytes = n * (b if name == "det.count" else b * K)
            _ffi.check(_ffi.lib().isegmi_engine_download_async(self._h, slot, C.c_void_p(pinned.ptr.value + off), self._buffer_info(name)[0], nbytes))
            off += nbytes

    def unpack_detections(self, pinned, n):
        """-> copies of (count [n], box [n, cap, 4], score [n, cap], label [n, cap]) out of a block download_detections_async filled."""
        K = self.cfg.det_cap
        out, off = [], 0
        for name, b, dt in self._DET:
            nbytes = n * (b if name == "det.count" else b * K)
            a = np.array(pinned.array[off:off + nbytes]).view(dt)
            out.append(a if name == "det.count" else a.reshape((n, K, 4) if name == "det.box" else (n, K)))
            off += nbytes
        return out
