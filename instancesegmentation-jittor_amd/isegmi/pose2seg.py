"""Pose2Seg inference (the reference README's section 2.2, `python test.py --weights last.pkl --coco --OCHuman`): images plus COCO keypoints
in, one mask per person out.  The contract is DESIGN.md section 9.

    net = Pose2Seg(state_dict, Pose2SegConfig(), max_batch=8, max_instances=32)
    masks = net([img_bgr_u8, ...], [kpts (n, 17, 3), ...])      # per image a list of (h, w) uint8 masks
    results = test(net, images, keypoints, image_ids)            # COCO segmentation dicts, category 1, score 1.0

Without annotations a Keypoint R-CNN finds the persons: its keypoints reach Pose2Seg on the device, only the person counts
come to the host.

    pipe = KeypointPose2Seg(keypoint_model, net, person_threshold=0.5, keypoint_threshold=2.0)
    for masks, boxes, scores, kpts in pipe([img_bgr_u8, ...]): ...   # per image: (h, w) uint8 masks, tight boxes, box scores, the (n, 17, 3) keypoints used
    results = test_from_images(pipe, images, image_ids)          # the same dicts, score = the detection's box score

The model runs on an engine of model_kind 3 (csrc/pose2seg.cpp, isegmi_pose2seg_forward): the fp32 MFMA convolutions for the ResNet-50 body,
the FPN top-down chain to P2 and the SegModule; csrc/pose2seg_ops.hip for the letterbox, the template fit, Affine-Align, the skeleton
features and the fused softmax + reverse warp.  Its masks, boxes, RLE and record block are the other models' (isegmi_engine_rle,
isegmi_engine_pack_coco_records, isegmi.pipeline.run_record_loop).  There is no CPU fallback.  Nothing here imports torch.
"""
import ctypes as C
from dataclasses import dataclass, replace

import numpy as np

from . import _ffi
from .engine import Engine
from .weights import fold_batchnorm, to_krsc

S_IN, S_FEAT, S_ALIGN = 512, 128, 64
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


@dataclass
class Pose2SegConfig:
    """The switches where the upstream recall is uncertain; the defaults are the recalled upstream behaviour."""
    warp_round_u8: int = 1          # round the letterboxed pixel to u8 (cv2.warpAffine returns uint8); 0 keeps it float
    swap_rb: int = 0                # 1: reverse the channel order before normalising (the caller hands RGB)
    fpn_upsample: str = "nearest"   # FPN top-down: "nearest" x2 or "bilinear" (align_corners=False)
    align_corners: int = 0          # Affine-Align's affine_grid / grid_sample; 1 = the PyTorch 0.4 era behaviour
    cat_skeleton: int = 1           # concatenate the 55 skeleton channels to the aligned features
    fp16: bool = False              # refused: fp32 only
    graph: int = 0                  # refused: no captured-graph replay for this model
    max_instances: int = 32         # persons per image: the record capacity K; more raise

    @property
    def det_cap(self):
        return self.max_instances


def letterbox_matrix(h, w):
    """m1: the image into the 512 x 512 input plane, centred at the largest scale that fits (fp64, row-major 2 x 3)."""
    s = min(512.0 / w, 512.0 / h)
    return [s, 0.0, 256.0 - s * w / 2.0, 0.0, s, 256.0 - s * h / 2.0]


def letterbox_inverse(m1):
    s, tx, ty = m1[0], m1[2], m1[5]
    return [1.0 / s, 0.0, -tx / s, 0.0, 1.0 / s, -ty / s]


def _conv(sd, name, bn=None, bias=False, cin_pad=None):
    w = to_krsc(sd[name + ".weight"])
    if cin_pad is not None and w.shape[3] < cin_pad:
        w = np.concatenate([w, np.zeros(w.shape[:3] + (cin_pad - w.shape[3],), np.float32)], axis=3)
    if bn is not None:
        sc, sh = fold_batchnorm(sd, bn)
        return w, sc, sh
    return (w, None, np.asarray(sd[name + ".bias"], np.float32)) if bias else (w, None, None)


def _count(sd, prefix):
    n = 0
    while prefix + "%d.conv1.weight" % n in sd:
        n += 1
    return n


def engine_layers(sd, cfg):
    """The state dict (weights.pose2seg_state_dict names) as the engine's layers: [(name, KRSC weight, scale, shift)] with BN folded, the stem
    padded to 4 input channels and segnet.conv1 zero-padded to the RoI tensor's channel count.  Widths and block counts come from the shapes."""
    out = []

    def bneck(nm):
        out.extend([(nm + ".conv1",) + _conv(sd, nm + ".conv1", nm + ".bn1"), (nm + ".conv2",) + _conv(sd, nm + ".conv2", nm + ".bn2"),
                    (nm + ".conv3",) + _conv(sd, nm + ".conv3", nm + ".bn3")])
        if nm + ".downsample.0.weight" in sd:
            out.append((nm + ".downsample.0",) + _conv(sd, nm + ".downsample.0", nm + ".downsample.1"))

    out.append(("backbone.conv1",) + _conv(sd, "backbone.conv1", "backbone.bn1", cin_pad=4))
    for li in range(4):
        pre = "backbone.layers.%d." % li
        if _count(sd, pre) == 0:
            raise ValueError("no blocks in " + pre)
        for b in range(_count(sd, pre)):
            bneck(pre + "%d" % b)
    for l in (2, 3, 4, 5):
        out.append(("fpn.lateral%d" % l,) + _conv(sd, "fpn.lateral%d" % l, bias=True))
    out.append(("fpn.output2",) + _conv(sd, "fpn.output2", bias=True))
    C = sd["fpn.output2.weight"].shape[0]
    need = C + 55 if cfg.cat_skeleton else C
    if sd["segnet.conv1.weight"].shape[1] != need:
        raise ValueError("segnet.conv1 takes %d input channels; cat_skeleton=%d needs %d" % (sd["segnet.conv1.weight"].shape[1], cfg.cat_skeleton, need))
    out.append(("segnet.conv1",) + _conv(sd, "segnet.conv1", "segnet.bn1", cin_pad=C + 64 if cfg.cat_skeleton else C))
    for st in ("segnet.stage1.", "segnet.stage2."):
        for b in range(_count(sd, st)):
            bneck(st + "%d" % b)
    out.append(("segnet.conv_out",) + _conv(sd, "segnet.conv_out", bias=True))
    return out


class Pose2Seg(Engine):
    """Pose2Seg(state_dict, cfg, max_batch, max_instances, device): upstream's `model([img], [kpts], [masks])` call shape on an engine of
    model_kind 3 (isegmi_pose2seg_forward).  Images are uint8 [h, w, 3] in the caller's channel order (upstream: cv2.imread BGR); keypoints
    (n, 17, 3) COCO (x, y, v).  Images and keypoints go up through pinned memory on the engine's copy stream (two slots)."""
    KIND = 3
    _NAMES = {"p2": "p2s.p2", "roi": "p2s.roi", "logits": "p2s.logits", "fit": "p2s.fit", "masks": "det.masks", "boxes": "det.box_resized",
              "scores": "det.score", "labels": "det.label", "count": "det.count"}

    def __init__(self, state_dict, cfg=None, max_batch=8, max_instances=None, device=0):
        cfg = replace(cfg or Pose2SegConfig())
        if max_instances is not None:
            cfg.max_instances = int(max_instances)
        self.cfg = cfg
        if cfg.fp16:
            raise ValueError("Pose2Seg: fp16 is not supported (fp32 only)")
        if cfg.graph:
            raise ValueError("Pose2Seg: graph capture is not supported for this model (graph must be 0)")
        if cfg.fpn_upsample not in ("nearest", "bilinear"):
            raise ValueError("fpn_upsample must be 'nearest' or 'bilinear'")
        if not (1 <= max_batch and 1 <= cfg.max_instances and max_batch * cfg.max_instances <= 65535):
            raise ValueError("max_batch / max_instances out of range")
        self.max_batch, self.max_instances = int(max_batch), cfg.max_instances
        templates = np.ascontiguousarray(state_dict["pose_templates"], np.float32)
        if templates.ndim != 3 or templates.shape[1:] != (17, 3) or not 1 <= templates.shape[0] <= 64:
            raise ValueError("pose_templates must be [T][17][3] with 1 <= T <= 64, got %s" % (templates.shape,))
        layers = engine_layers(state_dict, cfg)
        self._create(device, self.max_batch, S_IN, S_IN)
        for k, v in (("max_instances", cfg.max_instances), ("cat_skeleton", cfg.cat_skeleton), ("align_corners", cfg.align_corners),
                     ("warp_round_u8", cfg.warp_round_u8), ("swap_rb", cfg.swap_rb), ("fpn_bilinear", cfg.fpn_upsample == "bilinear")):
            self.set_param(k, float(v))
        for name, w, sc, sh in layers:
            self._set_conv_krsc(name, w, sc, sh)
        self._set_tensor("pose_templates", templates)
        self._pin = [[None, None], [None, None]]   # [slot][images, keypoints]
        self._dev = [[None, None], [None, None]]
        self._slot = 0
        self.last = {}

    def _staging(self, slot, which, nbytes):
        """pinned source + device destination of slot `slot` (which: 0 images, 1 keypoints), grown on demand"""
        pin, dev = self._pin[slot][which], self._dev[slot][which]
        if pin is None or pin.nbytes < nbytes:
            self.sync()   # no upload from the old buffers is still in flight
            for b in (pin, dev):
                if b is not None:
                    b.free()
            n = max(int(nbytes), 64)
            pin = self._pin[slot][which] = _ffi.PinnedBuffer((n,), np.uint8)
            dev = self._dev[slot][which] = _ffi.DeviceBuffer((n,), np.uint8)
        return pin, dev

    # -- the model ---------------------------------------------------------------------------------------------------------------------
    def _image_sizes(self, images):
        hw = []
        for im in images:
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise TypeError("Pose2Seg takes uint8 [h, w, 3] images")
            hw.append(im.shape[:2])
        return hw

    def _upload_images(self, images, hw, slot):
        """the images back to back through slot `slot`'s pinned buffer on the copy stream -> the device staging buffer"""
        nbytes = sum(h * w * 3 for h, w in hw)
        pin, dev = self._staging(slot, 0, nbytes)
        off = 0
        for im in images:
            a = np.ascontiguousarray(im).reshape(-1)
            pin.array[off:off + a.size] = a
            off += a.size
        _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, dev.ptr, pin.ptr, nbytes))
        return dev

    def body(self, images, slot=None):
        """The half of the forward that needs no persons (isegmi_pose2seg_body): upload, letterbox, ResNet body, FPN down to P2.  persons() ends the step."""
        N = len(images)
        if not 1 <= N <= self.max_batch:
            raise ValueError("batch of %d images; this model takes 1..%d" % (N, self.max_batch))
        hw = self._image_sizes(images)
        slot = self._slot if slot is None else slot
        self._slot = 1 - slot
        dev = self._upload_images(images, hw, slot)
        hwa = np.ascontiguousarray(hw, np.int32)
        _ffi.check(_ffi.lib().isegmi_pose2seg_body(self._h, dev.ptr, hwa.ctypes.data_as(C.c_void_p), N))
        self._body = dict(N=N, K=self.max_instances, hw=[tuple(x) for x in hw], Hmax=int(hwa[:, 0].max()), Wmax=int(hwa[:, 1].max()))
        return self._body

    def persons(self, d_kpts, counts, d_scores=None, producer_stream=None):
        """The other half (isegmi_pose2seg_persons) of the batch body() enqueued: d_kpts a device buffer [R][17][3] (or its pointer), counts [N] on the
        host; d_scores [N][max_instances] on the device become det.score of the live slots; producer_stream: the stream that wrote both."""
        L = getattr(self, "_body", None)
        if L is None:
            raise RuntimeError("persons() before body()")
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        if counts.shape[0] != L["N"]:
            raise ValueError("one person count per image of the body's batch (%d), got %d" % (L["N"], counts.shape[0]))
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        self._body = None
        _ffi.check(_ffi.lib().isegmi_pose2seg_persons(self._h, ptr(d_kpts), ptr(d_scores), counts.ctypes.data_as(C.c_void_p), producer_stream))
        self.last = dict(L, R=int(counts.sum()), counts=counts)
        return self.last

    def forward(self, images, keypoints, slot=None):
        """Enqueues upload + the whole forward of one batch (isegmi_pose2seg_forward); results stay in the engine's buffers."""
        N = len(images)
        if not 1 <= N <= self.max_batch:
            raise ValueError("batch of %d images; this model takes 1..%d" % (N, self.max_batch))
        if len(keypoints) != N:
            raise ValueError("one keypoint array per image")
        kps = []
        for kp in keypoints:
            k = np.zeros((0, 17, 3), np.float32) if kp is None or np.size(kp) == 0 else np.asarray(kp, np.float32)
            if k.ndim == 2:
                k = k[None]
            if k.ndim != 3 or k.shape[1:] != (17, 3):
                raise ValueError("keypoints of one image must be (n, 17, 3) COCO (x, y, v), got %s" % (k.shape,))
            if k.shape[0] > self.max_instances:
                raise ValueError("%d persons in one image: more than max_instances = %d" % (k.shape[0], self.max_instances))
            kps.append(k)
        hw = self._image_sizes(images)
        slot = self._slot if slot is None else slot
        self._slot = 1 - slot
        dev = self._upload_images(images, hw, slot)
        counts = np.array([k.shape[0] for k in kps], np.int32)
        R = int(counts.sum())
        dk = None
        if R:
            kall = np.ascontiguousarray(np.concatenate(kps), np.float32).view(np.uint8).reshape(-1)
            kpin, dk = self._staging(slot, 1, kall.size)
            kpin.array[:kall.size] = kall
            _ffi.check(_ffi.lib().isegmi_engine_upload_async(self._h, dk.ptr, kpin.ptr, kall.size))
        hwa = np.ascontiguousarray(hw, np.int32)
        _ffi.check(_ffi.lib().isegmi_pose2seg_forward(self._h, dev.ptr, hwa.ctypes.data_as(C.c_void_p), None if dk is None else dk.ptr,
                                                      counts.ctypes.data_as(C.c_void_p), N))
        self.last = dict(N=N, K=self.max_instances, R=R, hw=[tuple(x) for x in hw], counts=counts, Hmax=int(hwa[:, 0].max()), Wmax=int(hwa[:, 1].max()))
        return self.last

    def read(self, name, shape, dtype=np.float32):
        """Copy the first prod(shape) elements of a buffer of the last forward to the host (tests, diagnostics); p2 / roi / logits / fit /
        masks / boxes / scores / labels / count."""
        if name in ("roi", "logits", "fit") and not self.last.get("R"):
            raise ValueError("the last batch had no person: there is no %s" % name)
        self.sync()
        p, nb = self._buffer_info(self._NAMES.get(name, name))[:2]
        out = np.empty(shape, dtype)
        if out.nbytes > nb:
            raise ValueError("%s holds %d bytes, %d asked" % (name, nb, out.nbytes))
        if out.nbytes:
            _ffi.check(_ffi.lib().isegmi_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def collect(self):
        """The last forward's masks: per image a list of (h, w) uint8 arrays, and the tight boxes [n, 4] (xyxy, right / bottom exclusive)."""
        L = self.last
        N, K, Hm, Wm = L["N"], L["K"], L["Hmax"], L["Wmax"]
        planes = self.read("masks", (N, K, Hm, Wm), np.uint8)
        boxes = self.read("boxes", (N, K, 4))
        out_m, out_b = [], []
        for n, (h, w) in enumerate(L["hw"]):
            c = int(L["counts"][n])
            out_m.append([planes[n, k, :h, :w].copy() for k in range(c)])
            out_b.append(boxes[n, :c].copy())
        return out_m, out_b

    def __call__(self, batchimgs, batchkpts, batchmasks=None):
        """upstream's model(batchimgs, batchkpts, batchmasks): batchmasks is accepted and ignored (inference)."""
        self.forward(batchimgs, batchkpts)
        return self.collect()[0]

    def close(self):
        super().close()
        for row in getattr(self, "_pin", []) + getattr(self, "_dev", []):
            for b in row:
                if b is not None:
                    b.free()
        self._pin, self._dev = [], []


def test(net, images, keypoints, image_ids, batch_size=None, rank=0, world=1):
    """upstream test.py's COCO output: for every person dict(image_id, category_id 1, bbox, segmentation RLE at the image's size, score 1.0).
    images: list of uint8 [h, w, 3] (or a callable i -> image); keypoints: list of (n_i, 17, 3).  The step loop is the other models'
    (isegmi.pipeline.run_record_loop): forward, RLE on the device and one record block per step downloaded asynchronously; a step whose RLE
    overflows the capacities is redone with larger ones."""
    from .coco import results_from_records
    from .pipeline import run_record_loop
    bs = int(batch_size or net.max_batch)
    assert bs <= net.max_batch
    load = images if callable(images) else (lambda i: images[i])
    n_img = len(image_ids)
    batches = [list(range(j, min(j + bs, n_img))) for j in range(0, n_img, bs)]
    hws = {}
    per_image = [None] * n_img

    def enqueue(step, slot):
        j = step * world + rank
        if j >= len(batches):
            return False
        b = batches[j]
        ims = [load(i) for i in b]
        for i, im in zip(b, ims):
            hws[i] = np.asarray(im).shape[:2]
        net.forward(ims, [keypoints[i] for i in b], slot=slot)
        net.rle_device([hws[i] for i in b])
        return True

    def consume(step, recs):
        for r, rec in enumerate(recs):
            j = step * world + r
            if j >= len(batches):
                continue
            b = batches[j]
            res = results_from_records(rec, [image_ids[i] for i in b] + [None] * (bs - len(b)), [hws[i] for i in b] + [(1, 1)] * (bs - len(b)),
                                       3, net.max_instances)
            by_id = {}
            for d in res:
                by_id.setdefault(d["image_id"], []).append(d)
            for i in b:
                per_image[i] = by_id.get(image_ids[i], [])

    run_record_loop(net, bs, -(-len(batches) // world), enqueue, consume, rank, world)
    return [d for r in per_image if r for d in r]


class KeypointPose2Seg:
    """KeypointPose2Seg(keypoint_model, pose2seg_net, person_threshold=0.5, keypoint_threshold=2.0): images in, person masks out.
    keypoint_model is a Keypoint R-CNN engine (isegmi.maskrcnn.MaskRCNN with MODEL.KEYPOINT_ON), pose2seg_net a Pose2Seg; the detector's keypoints reach
    Pose2Seg on the device (isegmi_engine_pose_handoff: detections with score > person_threshold, the best max_instances of an image by score, a keypoint
    visible where its logit > keypoint_threshold) -- only the N person counts come to the host, while Pose2Seg's backbone already runs.  The defaults are
    the reference README's confidence_threshold and vis_keypoints' kp_thresh.  Images are uint8 [h, w, 3] BGR; the detector sees them resized as COCODemo
    resizes them (MIN_SIZE_TEST / MAX_SIZE_TEST of its config unless given), Pose2Seg the originals."""

    def __init__(self, keypoint_model, pose2seg_net, person_threshold=0.5, keypoint_threshold=2.0, min_image_size=None, max_image_size=None):
        det, net = keypoint_model, pose2seg_net
        if not getattr(det, "keypoint_on", False):
            raise ValueError("KeypointPose2Seg: the detector has no keypoint head (MODEL.KEYPOINT_ON False)")
        if int(det.cfg.NUM_KEYPOINTS) != 17:
            raise ValueError("KeypointPose2Seg: Pose2Seg takes COCO's 17 keypoints, the detector has num_keypoints = %d" % det.cfg.NUM_KEYPOINTS)
        self.det, self.net = det, net
        self.person_threshold, self.keypoint_threshold = float(person_threshold), float(keypoint_threshold)
        self.min_image_size = int(det.cfg.MIN_SIZE_TEST if min_image_size is None else min_image_size)
        self.max_image_size = int(det.cfg.MAX_SIZE_TEST if max_image_size is None else max_image_size)
        self.max_batch, self.max_instances = min(det.max_batch, net.max_batch), net.max_instances
        B, K = self.max_batch, self.max_instances
        # two slots of hand-off outputs: step t + 1's detector may write while Pose2Seg still reads step t's persons
        self._out = [dict(kpts=_ffi.DeviceBuffer((B * K, 17, 3)), score=_ffi.DeviceBuffer((B, K)), slot=_ffi.DeviceBuffer((B, K), np.int32),
                          count=_ffi.DeviceBuffer((B,), np.int32), pin=_ffi.PinnedBuffer((B,), np.int32), u8=None) for _ in range(2)]
        self._slot = 0
        self.last = {}

    # the record loop (isegmi.pipeline.run_record_loop) drives the Pose2Seg engine, where the results are
    KIND = Pose2Seg.KIND
    cfg = property(lambda self: self.net.cfg)

    def __getattr__(self, name):
        if name in ("set_param", "rle_device", "coco_record_bytes", "pack_coco_records", "download_async", "download_fence", "download_wait", "read"):
            return getattr(self.net, name)
        raise AttributeError(name)

    def sync(self):
        self.det.sync()
        self.net.sync()

    def forward(self, images_bgr_u8, slot=None):
        """Enqueues one batch: detector -> hand-off -> (Pose2Seg body, then the count download is waited for) -> Pose2Seg persons.  The results stay in the
        Pose2Seg engine's buffers (masks / boxes / scores / count; collect(), rle_device(), the record block)."""
        from .transforms import maskrcnn_resize_u8
        N = len(images_bgr_u8)
        if not 1 <= N <= self.max_batch:
            raise ValueError("batch of %d images; this pipeline takes 1..%d" % (N, self.max_batch))
        det, net, K = self.det, self.net, self.max_instances
        hw = net._image_sizes(images_bgr_u8)
        slot = self._slot if slot is None else int(slot)
        self._slot = 1 - slot
        o = self._out[slot]
        # this slot's last step (the one before last) is through: its hand-off buffers and both engines' pinned image buffers may be written again
        _ffi.check(_ffi.lib().isegmi_pose2seg_wait_persons(net._h, o["kpts"].ptr))
        resized = [maskrcnn_resize_u8(np.asarray(im), self.min_image_size, self.max_image_size) for im in images_bgr_u8]
        nbytes = sum(r.size for r in resized)
        if o["u8"] is None or o["u8"].nbytes < nbytes:
            self.sync()
            if o["u8"] is not None:
                o["u8"].free()
            o["u8"] = _ffi.PinnedBuffer((nbytes,), np.uint8)
        off = 0
        for r in resized:
            o["u8"].array[off:off + r.size] = r.reshape(-1)
            off += r.size
        det.upload_u8_async(o["u8"], [r.shape[:2] for r in resized], slot)
        det.forward_device(N, slot)
        det.set_output_sizes([(w, h) for h, w in hw])   # the keypoints leave in the originals' coordinates, as the keypoint records do
        producer = det.results_stream()
        ratios = det.pose_handoff(self.person_threshold, self.keypoint_threshold, K, o["kpts"], o["score"], o["slot"], o["count"])
        det.download_async(slot, o["pin"], o["count"], N * 4)
        net.body(images_bgr_u8, slot)                  # enqueued BEFORE the wait: the counts come down behind the 512 x 512 backbone
        det.download_wait(slot)
        counts = np.array(o["pin"].array[:N], np.int32)
        net.persons(o["kpts"], counts, o["score"], producer)
        self.last = dict(net.last, slot=slot, ratios=ratios)
        return self.last

    def collect(self):
        """-> per image (masks [list of (h, w) uint8], tight boxes [n, 4], scores [n], keypoints [n, 17, 3] as Pose2Seg took them) of the last forward"""
        L, K = self.last, self.max_instances
        masks, boxes = self.net.collect()
        N, counts = L["N"], L["counts"]
        scores = self.net.read("scores", (N, K))
        o = self._out[L["slot"]]
        kp = o["kpts"].numpy()[:int(counts.sum())]
        off = np.concatenate([[0], np.cumsum(counts)])
        return [(masks[n], boxes[n], scores[n, :int(counts[n])].copy(), kp[off[n]:off[n + 1]].copy()) for n in range(N)]

    def source_slots(self):
        """[N, K] int32: the detection slot of the detector's last forward each person came from (-1: unused); joins boxes and labels back"""
        self.sync()
        return self._out[self.last["slot"]]["slot"].numpy()[:self.last["N"]]

    def __call__(self, images_bgr_u8):
        self.forward(images_bgr_u8)
        return self.collect()

    def close(self):
        for o in getattr(self, "_out", []):
            for b in o.values():
                if b is not None:
                    b.free()
        self._out = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def test_from_images(pipe, images, image_ids, batch_size=None, rank=0, world=1):
    """test() without annotations: a KeypointPose2Seg finds the persons.  -> COCO segmentation dicts (category 1, bbox = the mask's tight box) whose
    score is the detection's box score.  images: list of uint8 [h, w, 3] BGR (or a callable i -> image)."""
    from .coco import results_from_records
    from .pipeline import run_record_loop
    bs = int(batch_size or pipe.max_batch)
    assert bs <= pipe.max_batch
    load = images if callable(images) else (lambda i: images[i])
    n_img = len(image_ids)
    batches = [list(range(j, min(j + bs, n_img))) for j in range(0, n_img, bs)]
    hws = {}
    per_image = [None] * n_img

    def enqueue(step, slot):
        j = step * world + rank
        if j >= len(batches):
            return False
        b = batches[j]
        ims = [load(i) for i in b]
        for i, im in zip(b, ims):
            hws[i] = np.asarray(im).shape[:2]
        pipe.forward(ims, slot=slot)
        pipe.rle_device([hws[i] for i in b])
        return True

    def consume(step, recs):
        for r, rec in enumerate(recs):
            j = step * world + r
            if j >= len(batches):
                continue
            b = batches[j]
            res = results_from_records(rec, [image_ids[i] for i in b] + [None] * (bs - len(b)), [hws[i] for i in b] + [(1, 1)] * (bs - len(b)),
                                       3, pipe.max_instances)   # kind 3 takes `score` from the record: here the persons' box scores
            by_id = {}
            for d in res:
                by_id.setdefault(d["image_id"], []).append(d)
            for i in b:
                per_image[i] = by_id.get(image_ids[i], [])

    run_record_loop(pipe, bs, -(-len(batches) // world), enqueue, consume, rank, world)
    return [d for r in per_image if r for d in r]


def coco_results(image_id, masks):
    """Host form of upstream's output records for one image: category_id 1, score 1.0, the RLE of every (h, w) mask (isegmi.coco.rle_encode)."""
    from .coco import rle_encode
    return [{"image_id": image_id, "category_id": 1, "segmentation": rle_encode(m), "score": 1.0} for m in masks]


def read_person_keypoints(path):
    """COCO person_keypoints json -> (images [dict(id, file_name, height, width)], {image_id: (n, 17, 3) float32}); crowd annotations skipped."""
    import json
    with open(path) as f:
        d = json.load(f)
    kp = {}
    for an in d.get("annotations", []):
        if an.get("iscrowd", 0) != 0 or an.get("category_id", 1) != 1 or "keypoints" not in an:
            continue
        kp.setdefault(an["image_id"], []).append(np.asarray(an["keypoints"], np.float32).reshape(17, 3))
    out = {i: np.stack(v) for i, v in kp.items()}
    return list(d.get("images", [])), out
