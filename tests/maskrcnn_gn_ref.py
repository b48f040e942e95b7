"""CPU reference of the GroupNorm Mask R-CNN forward (TEST INFRASTRUCTURE ONLY): [UPSTREAM-RECALL] maskrcnn-benchmark's
gn_baselines/e2e_mask_rcnn_R_50_FPN_1x_gn, composed from the oracle's ops (oracle/ora.py) and the GroupNorm restatement in the
kernel's summation order (tests/groupnorm_ref.gn_kernel_order), so the engine is compared bit for bit.  Consumes the upstream-named state dict
(weights.maskrcnn_state_dict(gn=True)) as is.  A convolution in front of a GroupNorm runs bare: no bias, no activation."""
import numpy as np

from oracle import ora
from oracle.maskrcnn_ref import MaskRCNNRef, cell_anchors, grid_anchors

from groupnorm_ref import gn_kernel_order


def _krsc(w):
    return np.ascontiguousarray(np.transpose(np.asarray(w, np.float32), (0, 2, 3, 1)))


class MaskRCNNGNRef:
    def __init__(self, sd, depth=50, num_groups=32, dim_per_gp=-1, eps=1e-5, stacked_convs=4, pre_nms=1000, post_nms=1000, fpn_post=1000,
                 det_per_img=100, gn=gn_kernel_order):
        self.sd, self.depth, self.num_groups, self.dim_per_gp, self.eps, self.nconv = sd, depth, num_groups, dim_per_gp, eps, stacked_convs
        self.pre_nms, self.post_nms, self.fpn_post, self.dpi = pre_nms, post_nms, fpn_post, det_per_img
        self._gn = gn
        self.feats = {}

    def gn(self, x, norm, residual=None, relu=False):
        C = x.shape[-1]
        groups = C // self.dim_per_gp if self.dim_per_gp > 0 else self.num_groups
        return self._gn(x, groups, self.sd[norm + ".weight"], self.sd[norm + ".bias"], self.eps, residual, relu)

    def conv_gn(self, x, conv, norm, stride, pad, relu, residual=None, w=None):
        w = _krsc(self.sd[conv + ".weight"]) if w is None else w
        return self.gn(ora.conv2d(x, w, stride, pad, None, None, None, 0), norm, residual, relu)

    def bottleneck(self, x, nm, stride, proj):
        """BottleneckWithGN, STRIDE_IN_1X1 False: the stride sits on the 3x3."""
        idt = self.conv_gn(x, nm + ".downsample.0", nm + ".downsample.1", stride, 0, False) if proj else x
        t = self.conv_gn(x, nm + ".conv1", nm + ".bn1", 1, 0, True)
        t = self.conv_gn(t, nm + ".conv2", nm + ".bn2", stride, 1, True)
        return self.conv_gn(t, nm + ".conv3", nm + ".bn3", 1, 0, True, residual=idt)

    def _cb(self, x, name, stride, pad, act):
        return ora.conv2d(x, _krsc(self.sd[name + ".weight"]), stride, pad, None, self.sd[name + ".bias"], None, act)

    def backbone_fpn(self, images_nhwc3):
        sd = self.sd
        x = np.asarray(images_nhwc3, np.float32)
        x4 = np.concatenate([x, np.zeros(x.shape[:3] + (1,), np.float32)], -1)
        w1 = _krsc(sd["backbone.body.stem.conv1.weight"])
        w1 = np.concatenate([w1, np.zeros(w1.shape[:3] + (1,), np.float32)], -1)
        x = ora.maxpool(self.conv_gn(x4, None, "backbone.body.stem.bn1", 2, 3, True, w=w1), 3, 2, 1)
        Cs = []
        for li, nb in enumerate((3, 4, 23 if self.depth == 101 else 6, 3), 1):
            for b in range(nb):
                x = self.bottleneck(x, "backbone.body.layer%d.%d" % (li, b), 2 if (b == 0 and li > 1) else 1, b == 0)
            Cs.append(x)
        last = self.conv_gn(Cs[3], "backbone.fpn.fpn_inner4.0", "backbone.fpn.fpn_inner4.1", 1, 0, False)
        P = [None, None, None, self.conv_gn(last, "backbone.fpn.fpn_layer4.0", "backbone.fpn.fpn_layer4.1", 1, 1, False)]
        for l in (2, 1, 0):
            lat = self.conv_gn(Cs[l], "backbone.fpn.fpn_inner%d.0" % (l + 1), "backbone.fpn.fpn_inner%d.1" % (l + 1), 1, 0, False)
            last = ora.upsample_nearest2x_add(last, lat)
            P[l] = self.conv_gn(last, "backbone.fpn.fpn_layer%d.0" % (l + 1), "backbone.fpn.fpn_layer%d.1" % (l + 1), 1, 1, False)
        P.append(ora.maxpool(P[3], 1, 2, 0))
        self.feats = dict(C2=Cs[0], C5=Cs[3], P2=P[0], P3=P[1], P4=P[2], P5=P[3], P6=P[4])
        return P

    def xconv1fc(self, feat):
        """FPNXconv1fcFeatureExtractor on pooled [R, 7, 7, 256] features -> (features after the xconvs, fc6 output [R, 1, 1, MLP_HEAD_DIM])."""
        sd, fx = self.sd, "roi_heads.box.feature_extractor"
        for i in range(self.nconv):
            feat = self.conv_gn(feat, "%s.xconvs.%d" % (fx, 3 * i), "%s.xconvs.%d" % (fx, 3 * i + 1), 1, 1, True)
        w6 = sd[fx + ".fc6.weight"].astype(np.float32)
        w6k = np.ascontiguousarray(w6.reshape(w6.shape[0], feat.shape[-1], 7, 7).transpose(0, 2, 3, 1))
        return feat, ora.conv2d(feat, w6k, 1, 0, None, sd[fx + ".fc6.bias"], None, 1)

    def _pool(self, P, n, boxes, res):
        strides = (4, 8, 16, 32)
        lv = ora.level_map(boxes)
        out = np.zeros((boxes.shape[0], res, res, 256), np.float32)
        for k in range(2, 6):
            idx = np.nonzero(lv == k)[0]
            if len(idx):
                rois = np.concatenate([np.full((len(idx), 1), n, np.float32), boxes[idx]], 1)
                out[idx] = ora.roi_align(P[k - 2], rois, 1.0 / strides[k - 2], res, res, 2, 0)
        return out

    def forward(self, images_nhwc3, image_hw):
        sd = self.sd
        P = self.backbone_fpn(images_nhwc3)
        N = P[0].shape[0]
        strides, sizes = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512)
        lvl_out = [[] for _ in range(N)]
        for l, p in enumerate(P):
            t = self._cb(p, "rpn.head.conv", 1, 1, 1)
            logits = self._cb(t, "rpn.head.cls_logits", 1, 0, 0)
            deltas = self._cb(t, "rpn.head.bbox_pred", 1, 0, 0)
            anc = grid_anchors(p.shape[1], p.shape[2], strides[l], cell_anchors(strides[l], sizes[l]))
            for n in range(N):
                lvl_out[n].append(ora.rpn_level(logits[n].reshape(-1), deltas[n].reshape(-1, 4), anc, self.pre_nms, self.post_nms, 0.7, 0.0,
                                                float(image_hw[n][1]), float(image_hw[n][0]), 0))
        dets = []
        for n in range(N):
            b = np.concatenate([q[0] for q in lvl_out[n]], 0); s = np.concatenate([q[1] for q in lvl_out[n]], 0)
            ts, ti = ora.topk(s, min(self.fpn_post, len(s)))
            pr = b[ti]
            R = pr.shape[0]
            xf, f6 = self.xconv1fc(self._pool(P, n, pr, 7))
            md = f6.shape[-1]
            cls = ora.conv2d(f6, sd["roi_heads.box.predictor.cls_score.weight"].reshape(81, 1, 1, md), 1, 0, None,
                             sd["roi_heads.box.predictor.cls_score.bias"], None, 0).reshape(R, 81)
            reg = ora.conv2d(f6, sd["roi_heads.box.predictor.bbox_pred.weight"].reshape(324, 1, 1, md), 1, 0, None,
                             sd["roi_heads.box.predictor.bbox_pred.bias"], None, 0).reshape(R, 324)
            db, ds, dl = ora.box_postprocess(cls, reg, pr, float(image_hw[n][1]), float(image_hw[n][0]), 0.05, 0.5, self.dpi, 0, self.dpi)
            D = db.shape[0]
            m28 = np.zeros((D, 28, 28), np.float32)
            if D:
                mf = self._pool(P, n, db, 14)
                for i in range(1, 5):
                    nm = "roi_heads.mask.feature_extractor.mask_fcn%d" % i
                    mf = self.conv_gn(mf, nm + ".0", nm + ".1", 1, 1, True)
                up = ora.deconv2x2(mf, sd["roi_heads.mask.predictor.conv5_mask.weight"].astype(np.float32), sd["roi_heads.mask.predictor.conv5_mask.bias"], 1)
                m28 = ora.mask_logits_select(up.reshape(D, 784, 256), sd["roi_heads.mask.predictor.mask_fcn_logits.weight"].reshape(81, 256),
                                             sd["roi_heads.mask.predictor.mask_fcn_logits.bias"], dl).reshape(D, 28, 28)
            dets.append(dict(box=db, score=ds, label=dl, mask28=m28, proposals=pr, proposal_scores=ts, xconv=xf))
        return dets

    paste = staticmethod(MaskRCNNRef.paste)
