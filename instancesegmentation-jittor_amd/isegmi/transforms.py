"""Real-image front end: the host-side transforms either side of the hot path.

Mask R-CNN: COCODemo.build_transform = Resize(min 800, max 1333, PIL bilinear) -> BGR 0..255 -> subtract
PIXEL_MEAN (M1; README.md:320-331 passes an HxWx3 uint8 BGR array).  Yolact: FastBaseTransform resizes to
550x550 (bilinear, align_corners=False, no aspect keep), normalises with BGR mean/std and flips to RGB (Y1).
"""
import numpy as np


def get_size(w, h, min_size=800, max_size=1333):
    """maskrcnn-benchmark transforms.Resize.get_size -> (oh, ow)."""
    size = min_size
    mn, mx = float(min(w, h)), float(max(w, h))
    if mx / mn * size > max_size:
        size = int(round(max_size * mn / mx))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return oh, ow


def maskrcnn_resize_u8(image_bgr_u8, min_size=800, max_size=1333):
    """HxWx3 uint8 BGR -> resized uint8 BGR (PIL bilinear, as torchvision F.resize on a PIL image; PIL rounds back to bytes)."""
    from PIL import Image
    h, w = image_bgr_u8.shape[:2]
    oh, ow = get_size(w, h, min_size, max_size)
    rgb = Image.fromarray(np.ascontiguousarray(image_bgr_u8[:, :, ::-1]))
    rgb = rgb.resize((ow, oh), Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(rgb, np.uint8)[:, :, ::-1])


def maskrcnn_resize(image_bgr_u8, min_size=800, max_size=1333):
    """The same as float32 BGR 0..255 (the input of prepare_images on the host path)."""
    return maskrcnn_resize_u8(image_bgr_u8, min_size, max_size).astype(np.float32)


def bilinear_resize(img, oh, ow):
    """F.interpolate(mode='bilinear', align_corners=False) on an HxWxC float array (numpy, host side)."""
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]

    def coef(o, i):
        src = np.maximum((np.arange(o, dtype=np.float32) + 0.5) * np.float32(i / o) - 0.5, 0)
        i0 = np.minimum(src.astype(np.int64), i - 1)
        i1 = np.minimum(i0 + 1, i - 1)
        l1 = (src - i0).astype(np.float32)
        return i0, i1, 1 - l1, l1
    y0, y1, ly0, ly1 = coef(oh, h)
    x0, x1, lx0, lx1 = coef(ow, w)
    top = img[y0][:, x0] * lx0[None, :, None] + img[y0][:, x1] * lx1[None, :, None]
    bot = img[y1][:, x0] * lx0[None, :, None] + img[y1][:, x1] * lx1[None, :, None]
    return top * ly0[:, None, None] + bot * ly1[:, None, None]


def yolact_transform(image_bgr_u8, size=550, darknet=False):
    """FastBaseTransform: resize to size x size, then the backbone's transform (ResNet: mean / std; darknet=True: x / 255), RGB."""
    from .yolact import darknet_base_transform, fast_base_transform
    x = bilinear_resize(np.asarray(image_bgr_u8, np.float32), size, size)[None]
    return darknet_base_transform(x) if darknet else fast_base_transform(x)


def letterbox_geometry(h, w, S_h, S_w):
    """YOLOv3 letterbox of an h x w image on an S_h x S_w canvas -> (gain, nh, nw, pad_x, pad_y): gain = min(S_h / h, S_w / w), the resized image
    (round(h gain), round(w gain)) sits centred; the left / top padding is the floor of half the slack."""
    gain = min(S_h / h, S_w / w)
    nh, nw = min(max(int(round(h * gain)), 1), S_h), min(max(int(round(w * gain)), 1), S_w)
    return gain, nh, nw, (S_w - nw) // 2, (S_h - nh) // 2


def yolo_letterbox(image_bgr_u8, S_h=416, S_w=416):
    """HxWx3 uint8 BGR -> (canvas [S_h, S_w, 3] float32 RGB in 0..1, (gain, pad_x, pad_y)): PIL bilinear resize (bytes, as maskrcnn_resize_u8), x / 255, no
    mean / std, centred on a canvas filled with 0.5."""
    from PIL import Image
    h, w = image_bgr_u8.shape[:2]
    gain, nh, nw, px, py = letterbox_geometry(h, w, S_h, S_w)
    rgb = Image.fromarray(np.ascontiguousarray(image_bgr_u8[:, :, ::-1]))
    if (nh, nw) != (h, w):
        rgb = rgb.resize((nw, nh), Image.BILINEAR)
    out = np.full((S_h, S_w, 3), 0.5, np.float32)
    out[py:py + nh, px:px + nw] = np.asarray(rgb, np.float32) / np.float32(255.0)
    return out, (gain, px, py)


def yolo_unletterbox(boxes_xyxy, geometry, h, w):
    """Canvas coordinates back to the original h x w image, in float32: (x - pad_x) / gain, (y - pad_y) / gain, clipped to [0, w] x [0, h]."""
    gain, px, py = geometry
    b = np.asarray(boxes_xyxy, np.float32).reshape(-1, 4)
    out = (b - np.asarray([px, py, px, py], np.float32)) / np.float32(gain)
    out[:, 0::2] = np.clip(out[:, 0::2], np.float32(0), np.float32(w))
    out[:, 1::2] = np.clip(out[:, 1::2], np.float32(0), np.float32(h))
    return out.astype(np.float32)


# -- PIL-exact resize on the device: the tables and the one-upload blob of isegmi_op_resample_u8 ---------------------------
RESAMPLE_MAX_KSIZE = 1025     # ISEGMI_RESAMPLE_MAX_KSIZE
RESAMPLE_ENTRY_WORDS = 16     # ISEGMI_RESAMPLE_ENTRY_WORDS
_TABLES = {}


def resample_ksize(I, O):
    """Taps per output sample of PIL's bilinear filter on an axis I -> O: 2 ceil(max(I / O, 1)) + 1."""
    import math
    return 2 * int(math.ceil(max(I / O, 1.0))) + 1


def resample_tables(I, O):
    """PIL's 8-bit bilinear coefficient tables of one axis I -> O (isegmi_resample_coeffs, host only): (bounds [O, 2] = (xmin, n), kk [O, ksize]) int32,
    read-only and cached by (I, O).  Raises for I, O < 1 and for downscales beyond the kernel's cap (ksize > RESAMPLE_MAX_KSIZE)."""
    import ctypes as C
    from . import _ffi
    key = (int(I), int(O))
    t = _TABLES.get(key)
    if t is None:
        ks = C.c_int()
        _ffi.check(_ffi.lib().isegmi_resample_coeffs(key[0], key[1], None, None, C.byref(ks)))
        bounds, kk = np.zeros((key[1], 2), np.int32), np.zeros((key[1], ks.value), np.int32)
        _ffi.check(_ffi.lib().isegmi_resample_coeffs(key[0], key[1], bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p), C.byref(ks)))
        bounds.setflags(write=False); kk.setflags(write=False)
        if len(_TABLES) >= 1024:
            _TABLES.clear()
        t = _TABLES[key] = (bounds, kk)
    return t


class ResamplePlan:
    """The layout of one blob [image tables of every view][coefficient tables][original pixels, back to back] that a batch's resizes need, from sizes alone.

    sizes_hw: (h, w) of every original, in the order their pixels are packed.  views: one list per launch of (image, Hout, Wout, dst_y, dst_x, hflip,
    plane) -- image indexes sizes_hw, the resized image sits at (dst_y, dst_x) of canvas plane `plane`.  The layout (offsets, nbytes) needs no table
    values; header() computes them (cached per (I, O)) and write() fills a uint8 buffer -- pinned memory or a numpy array -- for the single upload."""

    def __init__(self, sizes_hw, views):
        self.sizes = [(int(h), int(w)) for h, w in sizes_hw]
        self.views = [[tuple(int(v) for v in e) for e in view] for view in views]
        self.table_off, off = [], 0
        for view in self.views:
            self.table_off.append(off)
            off += len(view) * RESAMPLE_ENTRY_WORDS * 4
        self.coeff_off = off
        self._axes, words = {}, 0
        for view in self.views:
            for i, ho, wo, *_ in view:
                h, w = self.sizes[i]
                for I, O in ((w, wo), (h, ho)):
                    if (I, O) not in self._axes:
                        ks = resample_ksize(I, O)
                        if I < 1 or O < 1 or ks > RESAMPLE_MAX_KSIZE:
                            raise ValueError("resize %d -> %d: sizes are positive and a downscale stays within 512 (at most %d taps per sample)" % (I, O, RESAMPLE_MAX_KSIZE))
                        self._axes[(I, O)] = (words, ks)
                        words += O * (2 + ks)
        self.coeff_words = words
        self.src_off = self.coeff_off + words * 4
        self.image_off, off = [], 0
        for h, w in self.sizes:
            self.image_off.append(off)
            off += h * w * 3
        self.pixel_bytes = off
        self.nbytes = self.src_off + off
        self._header = None

    def header(self):
        """-> (uint8 [src_off] header bytes, [int32 [n, 16] table per view])"""
        if self._header is None:
            coeffs = np.zeros(self.coeff_words, np.int32)
            for (I, O), (off, ks) in self._axes.items():
                bounds, kk = resample_tables(I, O)
                assert kk.shape == (O, ks)
                coeffs[off:off + 2 * O] = bounds.reshape(-1)
                coeffs[off + 2 * O:off + O * (2 + ks)] = kk.reshape(-1)
            tables = []
            for view in self.views:
                t = np.zeros((len(view), RESAMPLE_ENTRY_WORDS), np.int32)
                for r, (i, ho, wo, dy, dx, flip, plane) in enumerate(view):
                    h, w = self.sizes[i]
                    (ch, ksh), (cv, ksv) = self._axes[(w, wo)], self._axes[(h, ho)]
                    so = self.image_off[i]
                    lo = so & 0xFFFFFFFF   # the int64 offset as two int32 words
                    t[r] = (lo - (1 << 32) if lo >= 1 << 31 else lo, so >> 32, h, w, ho, wo, dy, dx, ch, cv, ksh, ksv, 1 if flip else 0, plane, 0, 0)
                tables.append(t)
            head = np.concatenate([t.reshape(-1) for t in tables] + [coeffs]).view(np.uint8)
            assert head.nbytes == self.src_off
            self._header = (head, tables)
        return self._header

    def write(self, buf_u8, images):
        """Header and pixels into buf_u8 (a flat uint8 array of at least nbytes)."""
        head, _ = self.header()
        assert len(images) == len(self.sizes) and buf_u8.size >= self.nbytes
        buf_u8[:self.src_off] = head
        for im, off, (h, w) in zip(images, self.image_off, self.sizes):
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.shape != (h, w, 3):
                raise TypeError("an original image is HxWx3 uint8 of the size the plan was made for")
            buf_u8[self.src_off + off:self.src_off + off + im.size] = im.reshape(-1)
        return self.nbytes


def maskrcnn_resize_plan(sizes_hw, min_size=800, max_size=1333):
    """One view: every original resized by get_size, top-left on its own canvas plane (to_image_list).  -> (plan, resized hw [n, 2] int32)"""
    hw = np.array([get_size(w, h, min_size, max_size) for h, w in sizes_hw], np.int32).reshape(-1, 2)
    return ResamplePlan(sizes_hw, [[(i, hw[i, 0], hw[i, 1], 0, 0, 0, i) for i in range(len(sizes_hw))]]), hw
