"""References of the ResNeXt models (TEST INFRASTRUCTURE ONLY), composed from the oracle models by import: oracle.maskrcnn_ref.MaskRCNNRef and
tests/retinanet_ref.RetinaNetRef with two differences in the trunk -- conv2 of every bottleneck is the per-group reference of tests/conv_grouped_ref.py
(never split-K), and with stride_in_1x1 False a stage's stride sits on that 3x3 instead of on conv1.  Everything else (stem, FPN, RPN, heads, tails) is
the parents' code.  The seeded inputs and the reference forwards are computed once per process and never modified."""
import functools

import numpy as np

import conv_grouped_ref as gr
import retinanet_ref as rr
from oracle import ora
from oracle.maskrcnn_ref import MaskRCNNRef, _frozen_bn, _krsc

GROUPS, WIDTH = 32, 8
SEED = 1234
IMAGE_SEED = 20261003


class ResNeXtRef(MaskRCNNRef):
    def __init__(self, sd, groups=GROUPS, stride_in_1x1=False, **kw):
        super().__init__(sd, **kw)
        assert not self.fp16
        self.groups, self.stride_in_1x1 = int(groups), bool(stride_in_1x1)
        self._moved = 1   # the stride conv1 handed on to conv2

    def _cbn(self, x, conv, bn, stride, pad, act, residual=None, may_split=False):
        if conv.endswith(".conv1") and not self.stride_in_1x1:
            self._moved, stride = stride, 1
        if not conv.endswith(".conv2"):
            return super()._cbn(x, conv, bn, stride, pad, act, residual, may_split)
        stride, self._moved = stride * self._moved, 1
        w = _krsc(self.sd[conv + ".weight"])
        if w.shape[3] == x.shape[3]:   # a dense conv2 (groups 1)
            return super()._cbn(x, conv, bn, stride, pad, act, residual, may_split)
        assert w.shape[3] * self.groups == x.shape[3] == w.shape[0] and residual is None
        sc, sh = _frozen_bn(self.sd, bn, self.bn_eps)
        return gr.grouped_ref(x, w, self.groups, stride, sc, sh, None, act)


class RetinaNeXtRef(rr.RetinaNetRef):
    def __init__(self, sd, groups=GROUPS, stride_in_1x1=False, depth=50, **kw):
        super().__init__(sd, depth=depth, **kw)
        self.m = ResNeXtRef(sd, groups=groups, stride_in_1x1=stride_in_1x1, depth=depth)


@functools.lru_cache(maxsize=None)
def state_dict(depth=50, seed=SEED):
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(seed, depth, groups=GROUPS, width_per_group=WIDTH)


@functools.lru_cache(maxsize=None)
def retina_state_dict():
    from isegmi.weights import retinanet_state_dict
    return retinanet_state_dict(SEED, 50, groups=GROUPS, width_per_group=WIDTH)


def config(**kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return MaskRCNNConfig(**dict(dict(depth=50, CONV_BODY="R-50-FPN", NUM_GROUPS=GROUPS, WIDTH_PER_GROUP=WIDTH, STRIDE_IN_1X1=False), **kw))


def small_images():
    rng = np.random.default_rng(IMAGE_SEED)
    return [rng.uniform(0, 255, (250, 340, 3)).astype(np.float32), rng.uniform(0, 255, (256, 300, 3)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def small(stride_in_1x1=False, conv_split_k=0, n=2):
    """Mask R-CNN X-50-32x8d on the small canvas (256 x 352), the first n images.  -> (x, hw, ref, dets)"""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images(small_images())
    x, hw = x[:n], hw[:n]
    ref = ResNeXtRef(state_dict(), stride_in_1x1=stride_in_1x1, conv_split_k=conv_split_k)
    rd = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, rd


@functools.lru_cache(maxsize=None)
def retina_small():
    """RetinaNet X-50-32x8d at the size tests/retinanet_common.py uses (two images, canvas 256 x 352).  -> (x, hw, ref, dets)"""
    import retinanet_common as rc
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images(rc.small_images())
    ref = RetinaNeXtRef(retina_state_dict(), cap=128)
    dets = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, dets
