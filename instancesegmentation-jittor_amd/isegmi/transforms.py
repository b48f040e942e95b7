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
