"""CPU reference of darknet's [maxpool], the SPP block and the YOLOv3-SPP / YOLOv3-tiny forwards (TEST INFRASTRUCTURE ONLY): a numpy pool plus the oracle's ops
as tests/yolov3_ref.py composes them (ora.conv2d act 3, ora.topk, ora.nms).  It restates DESIGN.md 21 ([UPSTREAM-RECALL] the public yolov3-spp.cfg /
yolov3-tiny.cfg and darknet's maxpool_layer.c, unverified).

The keyword forks of maxpool_darknet that are NOT the model (start_shift, symmetric) exist for the discrimination checks of tests/test_yolo_variants_cpu.py."""
import functools

import numpy as np

import yolov3_ref as yr
from oracle import ora

F32 = np.float32
TINY_STRIDES = (32, 16)
TINY_ANCHORS = np.asarray([[(81, 82), (135, 169), (344, 319)], [(10, 14), (23, 27), (37, 58)]], F32)


def maxpool_darknet(x, size, stride, zero_pad=False, start_shift=0, symmetric=False):
    """x [N, H, W, C] -> [N, (H - 1) // stride + 1, (W - 1) // stride + 1, C].  The window of output o covers the inputs o * stride - (size - 1) // 2 + [0, size).
    The maximum is `m = v if v > m else m` from -inf over the taps: the largest non-NaN tap, -inf where there is none.  A tap outside the map is skipped
    (zero_pad False: darknet) or is +0.0 (zero_pad True: ZeroPad2d + MaxPool2d).  Forks: start_shift moves the window start; symmetric pads size // 2 on
    every side, as nn.MaxPool2d(size, stride, size // 2) would (another output size for an even window)."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    off = (size - 1) // 2 + start_shift
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if symmetric:
        off = size // 2
        Ho, Wo = (H + 2 * off - size) // stride + 1, (W + 2 * off - size) // stride + 1
    m = np.full((N, Ho, Wo, C), -np.inf, F32)
    for r in range(size):
        hi = np.arange(Ho) * stride - off + r
        for q in range(size):
            wi = np.arange(Wo) * stride - off + q
            inside = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
            v = x[:, np.clip(hi, 0, H - 1)][:, :, np.clip(wi, 0, W - 1)]
            if zero_pad:
                v = np.where(inside[None, :, :, None], v, F32(0))
                take = v > m
            else:
                take = inside[None, :, :, None] & (v > m)
            m = np.where(take, v, m)   # a NaN never compares greater
    return m


def spp_concat(x, zero_pad=False):
    """[mp13 | mp9 | mp5 | x]: darknet's route layers = -1, -3, -5, -6 over the three stride-1 pools of x."""
    x = np.asarray(x, F32)
    return np.ascontiguousarray(np.concatenate([maxpool_darknet(x, k, 1, zero_pad) for k in (13, 9, 5)] + [x], -1))


class YoloSppRef(yr.YoloV3Ref):
    """yolov3-spp: YoloV3Ref with spp_concat and head.0.spp between head.0.conv2 and head.0.conv3."""

    def __init__(self, sd, zero_pad=False, **kw):
        super().__init__(sd, **kw)
        self.zero_pad = zero_pad

    def heads(self, images):
        C = self.trunk(np.asarray(images, F32))
        x, out = C[2], []
        for s in range(3):
            for i in range(5):
                x = self._cbn(x, "head.%d.conv%d" % (s, i), "head.%d.bn%d" % (s, i), 1, i & 1, 3)
                if s == 0 and i == 2:
                    self.feats["spp_in"] = x
                    x = self._cbn(spp_concat(x, self.zero_pad), "head.0.spp", "head.0.spp_bn", 1, 0, 3)
            branch = x
            t = self._cbn(branch, "head.%d.conv5" % s, "head.%d.bn5" % s, 1, 1, 3)
            out.append(ora.conv2d(t, yr._krsc(self.sd["head.%d.conv6.weight" % s]), 1, 0, None, self.sd["head.%d.conv6.bias" % s], None, 0))
            if s < 2:
                r = self._cbn(branch, "head.%d.route" % (s + 1), "head.%d.route_bn" % (s + 1), 1, 0, 3)
                x = yr.concat_up2x(r, C[1 - s])
        self.feats.update(C=C, heads=out)
        return out


class YoloTinyRef(yr.YoloV3Ref):
    """yolov3-tiny on the unpadded 16-channel first map (the engine's zero channels add exact zeros to every sum)."""

    def __init__(self, sd, zero_pad=False, **kw):
        super().__init__(sd, **dict(dict(strides=TINY_STRIDES, anchors=TINY_ANCHORS), **kw))
        self.zero_pad = zero_pad

    def heads(self, images):
        x = np.asarray(images, F32)
        for i in range(7):
            x = self._cbn(x, "backbone.conv%d" % i, "backbone.bn%d" % i, 1, 1, 3)
            if i == 4:
                skip = x
            if i < 6:
                x = maxpool_darknet(x, 2, 2 if i < 5 else 1, self.zero_pad)
        branch = self._cbn(x, "head.0.conv0", "head.0.bn0", 1, 0, 3)
        t = self._cbn(branch, "head.0.conv1", "head.0.bn1", 1, 1, 3)
        out = [ora.conv2d(t, yr._krsc(self.sd["head.0.conv2.weight"]), 1, 0, None, self.sd["head.0.conv2.bias"], None, 0)]
        r = self._cbn(branch, "head.1.route", "head.1.route_bn", 1, 0, 3)
        t = self._cbn(yr.concat_up2x(r, skip), "head.1.conv0", "head.1.bn0", 1, 1, 3)
        out.append(ora.conv2d(t, yr._krsc(self.sd["head.1.conv1.weight"]), 1, 0, None, self.sd["head.1.conv1.bias"], None, 0))
        self.feats = dict(top=x, skip=skip, heads=out)
        return out


# ---- the engines' seeded weights, inputs and reference forwards, computed once and shared by the CPU and GPU tests
ENGINE_SEED = 1234
ENGINE_CANVASES = ((64, 96), (96, 64), (32, 32))
ENGINE_CONF = 0.03   # at 0.05 the single cell of the spp model's stride-32 level on a 32 x 32 canvas has no candidate


def engine_input(H, W, N=2):
    return np.random.default_rng(2000 + H).uniform(0, 1, (N, H, W, 3)).astype(F32)


@functools.lru_cache(None)
def engine_weights(variant):
    from isegmi.weights import yolov3_state_dict
    return yolov3_state_dict(ENGINE_SEED, variant=variant)


@functools.lru_cache(None)
def engine_reference(variant, H, W, zero_pad=False):
    """-> (the reference after forward (feats: heads, dec, total), detections) at conf_thresh ENGINE_CONF, everything else default."""
    ref = {"spp": YoloSppRef, "tiny": YoloTinyRef}[variant](engine_weights(variant), zero_pad=zero_pad, thr=ENGINE_CONF)
    return ref, ref.forward(engine_input(H, W))
