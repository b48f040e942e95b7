"""Reference of the deformable-convolution R-CNN models (TEST INFRASTRUCTURE ONLY), composed from the oracle model by import:
oracle.maskrcnn_ref.MaskRCNNRef with ONE difference -- conv2 of every bottleneck of the deformable stages is the oracle's unfused deformable convolution
(offset conv -> ora.deform_im2col -> ora.conv2d as a 1x1 over 9 C channels, bn2 folded, ReLU); the unmodulated form goes through deform_conv_cases.as27.
Everything else (stem, the other layers, FPN, RPN, heads, tails) is the parent's code.  tests/resnext_ref.py is the pattern.  The seeded inputs and the
reference forwards are computed once per process and never modified."""
import functools

import numpy as np

import deform_conv_cases as dc
from oracle import ora
from oracle.maskrcnn_ref import MaskRCNNRef, _frozen_bn, _krsc

SEED = 1234
IMAGE_SEED = 20261021


class MaskRCNNDcnRef(MaskRCNNRef):
    def __init__(self, sd, stage_with_dcn=(False, True, True, True), **kw):
        super().__init__(sd, **kw)
        assert not self.fp16
        self.dcn = tuple(bool(v) for v in stage_with_dcn)
        self.stage_out = {}   # "res2".."res5": the stage's last block output
        self.om = {}          # block name -> raw offset-conv output

    def _cbn(self, x, conv, bn, stride, pad, act, residual=None, may_split=False):
        li = int(conv.split(".layer")[1].split(".")[0]) if ".layer" in conv else 0
        if conv.endswith(".conv2") and li and self.dcn[li - 1]:
            sd = self.sd
            om = ora.conv2d(x, _krsc(sd[conv + ".offset.weight"]), stride, 1, None, np.asarray(sd[conv + ".offset.bias"], np.float32), None, 0)
            self.om[conv] = om
            sc, sh = _frozen_bn(sd, bn, self.bn_eps)
            y, _ = dc.reference(x, om, _krsc(sd[conv + ".conv.weight"]), stride, sc, sh, None, act)
        else:
            y = super()._cbn(x, conv, bn, stride, pad, act, residual, may_split)
        if conv.endswith(".conv3") and li:
            self.stage_out["res%d" % (li + 1)] = y   # the last block's write stays
        return y


@functools.lru_cache(maxsize=None)
def state_dict(stage_with_dcn=(0, 1, 1, 1), modulated=True, mask=True):
    from isegmi.weights import maskrcnn_state_dict
    return maskrcnn_state_dict(SEED, 50, mask=mask, stage_with_dcn=stage_with_dcn, modulated=modulated)


def config(stage_with_dcn=(False, True, True, True), modulated=True, **kw):
    from isegmi.maskrcnn import MaskRCNNConfig
    return MaskRCNNConfig(**dict(dict(depth=50, CONV_BODY="R-50-FPN", STAGE_WITH_DCN=tuple(bool(v) for v in stage_with_dcn), WITH_MODULATED_DCN=bool(modulated)), **kw))


def images(canvas):
    """Two images that pad to `canvas` (H, W)."""
    H, W = canvas
    rng = np.random.default_rng([IMAGE_SEED, H, W])
    return [rng.uniform(0, 255, (H - 6, W - 12, 3)).astype(np.float32), rng.uniform(0, 255, (H, W - 40, 3)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def small(canvas=(192, 256), n=2, stage_with_dcn=(0, 1, 1, 1), modulated=True):
    """-> (x, hw, ref, dets): the first n images on `canvas`, the reference model and its detections."""
    from isegmi.maskrcnn import prepare_images
    x, hw = prepare_images(images(canvas)[:n])
    assert x.shape[1:3] == tuple(canvas), x.shape
    ref = MaskRCNNDcnRef(state_dict(tuple(stage_with_dcn), modulated), stage_with_dcn=stage_with_dcn)
    rd = ref.forward(x, hw)
    x.setflags(write=False)
    return x, hw, ref, rd
