"""PIL's 8-bit bilinear resize (Resample.c) restated in numpy: the contract of DESIGN.md 24 and the reference of the resample tests.

Tables per axis I -> O, all in IEEE double (Python floats: no contraction):
    scale = I / O, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1, center = (xx + 0.5) scale,
    xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), I) - xmin,
    w[x] = tri((x + xmin - center + 0.5) * (1 / fs)), normalised by their sum in index order, k[x] = int(w[x] * 2^22 + 0.5).
Pixel: clip8((2^21 + sum_x p[xmin + x] k[x]) >> 22) in int32.  Image: the horizontal pass first, rounded to uint8, then the vertical pass over those
bytes; a pass whose sizes match is skipped.  Channels are independent.
"""
import math

import numpy as np

# (h, w, oh, ow): the shapes at which the restatement was checked against PIL when the contract was written
SHAPES = [(480, 640, 800, 1067), (427, 640, 800, 1199), (7, 5, 13, 11), (1, 1, 4, 4), (33, 47, 8, 9), (64, 64, 64, 31), (50, 37, 50, 80),
          (200, 300, 3, 1), (17, 2, 40, 1), (1000, 37, 9, 90)]
MAX_KSIZE = 1025   # the kernel's cap: downscales up to 512


def coeffs(I, O):
    """-> (bounds [O, 2] int32 = (xmin, n), kk [O, ksize] int32)"""
    scale = I / O
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds, kk = np.zeros((O, 2), np.int32), np.zeros((O, ksize), np.int32)
    for xx in range(O):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), I) - xmin
        w, ww = [], 0.0
        for x in range(n):
            t = abs((x + xmin - center + 0.5) * (1.0 / fs))
            w.append(1.0 - t if t < 1.0 else 0.0)
            ww += w[-1]
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * 4194304.0 + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, kk


_cache = {}


def tables(I, O):
    if (I, O) not in _cache:
        _cache[(I, O)] = coeffs(I, O)
    return _cache[(I, O)]


def _pass(img, O, axis):
    """One pass along `axis` (0 vertical, 1 horizontal) of an [H, W, C] uint8 image."""
    I = img.shape[axis]
    if I == O:
        return img
    bounds, kk = tables(I, O)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((O,) + src.shape[1:], np.uint8)
    for xx in range(O):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = np.full(src.shape[1:], 1 << 21, np.int32)
        for x in range(n):
            ss += src[xmin + x] * kk[xx, x]
        out[xx] = np.clip(ss >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img_u8, oh, ow):
    """Image.fromarray(img).resize((ow, oh), Image.BILINEAR) on an [H, W, C] uint8 array."""
    img = np.ascontiguousarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3
    return np.ascontiguousarray(_pass(_pass(img, ow, 1), oh, 0))


def resize_view(img_u8, oh, ow, hflip=False):
    """Epilogue (a): the resized bytes; hflip mirrors the RESIZED image (output column x shows resized column ow - 1 - x)."""
    r = resize(img_u8, oh, ow)
    return np.ascontiguousarray(r[:, ::-1]) if hflip else r


def canvas_f32(img_u8, oh, ow, Hpad, Wpad, dst_y=0, dst_x=0, mean=(0, 0, 0), std=(1, 1, 1), swap=False, fill=0.0, hflip=False):
    """Epilogue (b): ((float)p - mean[c]) / std[c] into channel (2 - c if swap else c) of an [Hpad, Wpad, 3] float32 canvas at (dst_y, dst_x), `fill` elsewhere."""
    r = resize_view(img_u8, oh, ow, hflip).astype(np.float32)
    v = (r - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    out = np.full((Hpad, Wpad, 3), np.float32(fill), np.float32)
    out[dst_y:dst_y + oh, dst_x:dst_x + ow] = v[:, :, ::-1] if swap else v
    return out


def patterns(h, w, seed=0):
    """The three image contents of the tests: all 255 (accumulator maximum), a 0 / 255 checkerboard, random bytes."""
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    board[:, :, 1] = 255 - board[:, :, 1]
    rnd = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return {"ones": np.full((h, w, 3), 255, np.uint8), "board": np.ascontiguousarray(board), "random": rnd}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
