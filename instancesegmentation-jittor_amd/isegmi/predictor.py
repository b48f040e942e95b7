"""COCODemo -- the predictor object of README.md:288-335, backed by libisegmi.

    coco_demo = COCODemo(cfg, min_image_size=800, confidence_threshold=0.5, state_dict=sd)
    predictions = coco_demo.run_on_opencv_image(image)     # image: HxWx3 uint8 BGR -> annotated HxWx3 uint8

`cfg` is a MaskRCNNConfig (the handful of inference constants the path needs, keyed like the yaml).
compute_prediction / select_top_predictions follow the upstream demo ([UPSTREAM-RECALL]);
overlay drawing is numpy + PIL (cv2 is not in the image): mask tint, box outline and the "class score" label upstream's
overlay_class_names writes at the box's top-left corner (PIL's built-in font instead of cv2.putText's Hershey face).
"""
import numpy as np

from .coco import COCO_CLASSES
from .maskrcnn import BoxList, MaskRCNN, MaskRCNNConfig
from .transforms import maskrcnn_resize_u8


class COCODemo:
    CATEGORIES = ("__background",) + COCO_CLASSES

    def __init__(self, cfg=None, min_image_size=800, confidence_threshold=0.5, state_dict=None, max_image_size=1333, device=0, max_batch=2,
                 fp16=False, render="host", bbox_aug=None, aug_canvas=None, resize="host"):
        """resize: "host" -- PIL resizes every image before its bytes go up; "device" -- the original bytes go up and isegmi_engine_resample_u8 resizes
        them, bit-identical to PIL.  bbox_aug: a BBoxAugConfig next to a MaskRCNNConfig (a yaml-keyed node carries its own TEST.BBOX_AUG); aug_canvas = (H, W): the engine's largest
        canvas under augmentation instead of the one derived from the scales."""
        from .retinanet import RetinaNetConfig
        if render not in ("host", "device"):
            raise ValueError("render: 'host' (numpy overlay of the downloaded masks) or 'device' (isegmi_engine_paint; DESIGN.md 22)")
        if resize not in ("host", "device"):
            raise ValueError("resize: 'host' (PIL on the host) or 'device' (isegmi_engine_resample_u8; DESIGN.md 24)")
        self.render, self.resize = render, resize
        if cfg is not None and not isinstance(cfg, (MaskRCNNConfig, RetinaNetConfig)):   # the yacs-shaped node of isegmi.config (README.md:313-324)
            from .config import is_bbox_aug, is_keypoint_rcnn, is_retinanet, to_bbox_aug_config, to_keypointrcnn_config, to_maskrcnn_config, to_retinanet_config
            retina = is_retinanet(cfg)
            to_two_stage = to_keypointrcnn_config if is_keypoint_rcnn(cfg) else to_maskrcnn_config   # MODEL.KEYPOINT_ON
            if is_bbox_aug(cfg) and not retina and not is_keypoint_rcnn(cfg):   # TEST.BBOX_AUG.ENABLED; the other two mappings refuse the key by name
                bbox_aug = to_bbox_aug_config(cfg)[1]
                to_two_stage = lambda c: to_bbox_aug_config(c)[0]
            if state_dict is None and getattr(cfg.MODEL, "WEIGHT", ""):
                w = cfg.MODEL.WEIGHT
                from .weights import random_maskrcnn_state_dict, retinanet_state_dict
                body = cfg.MODEL.BACKBONE.CONV_BODY
                depth = 101 if "101" in body else 50
                # MODEL.WEIGHT random: the seeded generator of the configured model (body, norm, MASK_ON, NUM_CLASSES, CLS_AGNOSTIC_BBOX_REG)
                rn = cfg.MODEL.RESNETS
                rnd = (lambda: retinanet_state_dict(1234, depth, groups=int(rn.get("NUM_GROUPS", 1)), width_per_group=int(rn.get("WIDTH_PER_GROUP", 64)))) if retina else (lambda: random_maskrcnn_state_dict(to_two_stage(cfg), 1234))
                state_dict = rnd() if w == "random" else dict(np.load(w))
            cfg = to_retinanet_config(cfg) if retina else to_two_stage(cfg)
        self.cfg = cfg or MaskRCNNConfig()
        self.is_retinanet = isinstance(self.cfg, RetinaNetConfig)   # MODEL.RETINANET_ON: boxes, scores and labels; no masks
        self.box_only = not self.is_retinanet and not self.cfg.MASK_ON   # MODEL.MASK_ON False: Faster R-CNN, the same
        self.bbox_aug, self.aug_canvas = bbox_aug, aug_canvas   # TEST.BBOX_AUG: every prediction is MaskRCNN.detect_aug's
        if bbox_aug is not None and (self.is_retinanet or not self.box_only or self.cfg.KEYPOINT_ON or self.cfg.is_c4 or fp16):
            raise ValueError("TEST.BBOX_AUG.ENABLED is built for the box-only fp32 FPN models (MODEL.MASK_ON False, MODEL.KEYPOINT_ON False, no C4 body, no RetinaNet)")
        if not self.is_retinanet and self.cfg.NUM_CLASSES != 81:      # labels of another class count have no COCO names
            self.CATEGORIES = ("__background",) + tuple("class %d" % i for i in range(1, self.cfg.NUM_CLASSES))
        if state_dict is None:
            raise ValueError("COCODemo needs weights: pass state_dict=... or set cfg.MODEL.WEIGHT to an .npz (or 'random'); "
                             "the reference's download URLs (README.md:266) cannot be fetched here")
        self.min_image_size, self.max_image_size = min_image_size, max_image_size
        self.confidence_threshold = confidence_threshold
        self.state_dict, self.device, self.max_batch, self.fp16 = state_dict, device, int(max_batch), bool(fp16)
        self._model = None

    def engine(self, max_batch=None):
        """THE engine of this predictor: weights packed once, every buffer sized once for the largest canvas the resize rule can produce
        (long side max_image_size, either orientation, rounded up to SIZE_DIVISIBILITY).  Each batch then runs on its own padded canvas,
        exactly as upstream's to_image_list pads it (results depend on the canvas: the RPN sees the padding)."""
        want = int(max_batch or self.max_batch)
        if self._model is not None and self._model.max_batch < want:
            self._model.close()
            self._model = None
        if self._model is None:
            d = self.cfg.SIZE_DIVISIBILITY
            m = -(-max(self.max_image_size, self.min_image_size) // d) * d
            mh = mw = m
            if self.bbox_aug is not None:   # the largest view the plain rule's aspect allows, or the caller's canvas
                from .maskrcnn import bbox_aug_engine_side
                mh = mw = bbox_aug_engine_side(self.cfg, self.bbox_aug, self.min_image_size, self.max_image_size)
                if self.aug_canvas is not None:
                    mh, mw = (-(-int(v) // d) * d for v in self.aug_canvas)
            if self.is_retinanet:
                from .retinanet import RetinaNet
                self._model = RetinaNet(self.state_dict, m, m, cfg=self.cfg, max_batch=want, device=self.device, fp16=self.fp16)
            else:
                self._model = MaskRCNN(self.state_dict, mh, mw, cfg=self.cfg, max_batch=want, device=self.device, fp16=self.fp16)
            self.memory = self._model.reserve()  # (weight bytes, activation / workspace bytes): the predictor's peak device memory
        return self._model

    def compute_prediction(self, original_image):
        """-> BoxList in ORIGINAL image coordinates with scores, labels and mask [n,1,H,W] uint8 (Masker output); RetinaNet and Faster R-CNN
        (MODEL.MASK_ON False): no mask field.  Keypoint R-CNN (MODEL.KEYPOINT_ON): keypoints [n,17,3] in original-image coordinates and keypoint_logits [n,17]."""
        h, w = original_image.shape[:2]
        model = self.engine()
        if self.bbox_aug is not None:   # TEST.BBOX_AUG: the views are resized from the original inside detect_aug
            (pred,) = model.detect_aug([original_image], self.bbox_aug, self.min_image_size, self.max_image_size, self.resize)
            return pred.resize((w, h))
        (pred,) = self._forward_one(model, original_image)
        if self.is_retinanet or self.box_only:
            return pred.resize((w, h))
        model.paste_device(h, w, [(w, h)])
        model.sync()
        n = len(pred)
        masks = model.fetch("det.masks", 1)[0, :n]
        out = pred.resize((w, h))
        out.add_field("mask", masks[:, None])
        return out

    def _forward_one(self, model, image):
        """One image through the front end and the forward.  resize="host": PIL, then the bytes cross PCIe and mean subtraction + padding (to_image_list)
        run on the GPU; "device": the original bytes cross and the resize runs there too."""
        if self.resize == "device":
            return model.detect_original([image], self.min_image_size, self.max_image_size)
        return model([maskrcnn_resize_u8(image, self.min_image_size, self.max_image_size)])

    def select_top_predictions(self, predictions):
        scores = predictions.get_field("scores")
        keep = np.nonzero(scores > self.confidence_threshold)[0]
        predictions = predictions[keep]
        order = np.argsort(-predictions.get_field("scores"), kind="stable")
        return predictions[order]

    def run_on_opencv_image(self, image):
        if self.render == "device":
            return self._run_on_device(image)
        predictions = self.select_top_predictions(self.compute_prediction(image))
        return self.overlay(image.copy(), predictions)

    def _run_on_device(self, image):
        """run_on_opencv_image with the painting on the device (render="device"): forward and paste as compute_prediction, but det.masks stays where
        the paste wrote it -- only the small detection arrays come back, the selection runs on them, and isegmi_engine_paint draws the selected
        detections in their selected order from their rows of det.masks (`slot`: the row before selection).  The image goes up and comes back once;
        the class names are written on the host, as overlay does.  Bit-identical to the host overlay."""
        from .render import demo_entries, keypoint_dots
        h, w = image.shape[:2]
        model = self.engine()
        if self.bbox_aug is not None:
            (pred,) = model.detect_aug([image], self.bbox_aug, self.min_image_size, self.max_image_size, self.resize)
        else:
            (pred,) = self._forward_one(model, image)
        with_masks = not (self.is_retinanet or self.box_only)
        if with_masks:
            model.paste_device(h, w, [(w, h)])   # on the results stream; the painter is ordered behind it
        pred = pred.resize((w, h))
        pred.add_field("slot", np.arange(len(pred), dtype=np.int64))
        predictions = self.select_top_predictions(pred)
        dots = keypoint_dots(predictions, self.KP_THRESH) if predictions.has_field("keypoints") else None
        out = model.paint_device(image, demo_entries(predictions, h, w, with_masks), dots)
        return self.overlay_class_names(out, predictions)

    @staticmethod
    def compute_colors_for_labels(labels):
        palette = np.array([2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1], np.int64)
        return ((np.asarray(labels, np.int64)[:, None] * palette) % 255).astype(np.uint8)

    def overlay(self, image, predictions):
        colors = self.compute_colors_for_labels(predictions.get_field("labels")) if len(predictions) else []
        masks = predictions.get_field("mask") if predictions.has_field("mask") else None
        H, W = image.shape[:2]
        for k in range(len(predictions)):
            c = colors[k].astype(np.float32)
            if masks is not None:
                m = masks[k, 0].astype(bool)
                image[m] = (0.5 * image[m] + 0.5 * c).astype(np.uint8)
            x1, y1, x2, y2 = (int(v) for v in predictions.bbox[k])
            x1, x2 = max(0, min(W - 1, x1)), max(0, min(W - 1, x2))
            y1, y2 = max(0, min(H - 1, y1)), max(0, min(H - 1, y2))
            image[y1:y2 + 1, [x1, x2]] = colors[k]
            image[[y1, y2], x1:x2 + 1] = colors[k]
        if predictions.has_field("keypoints"):
            self.overlay_keypoints(image, predictions)
        return self.overlay_class_names(image, predictions)

    KP_THRESH = 2.0   # [UPSTREAM-RECALL] demo/predictor.py vis_keypoints: kp_thresh

    def overlay_keypoints(self, image, predictions):
        """A 5 x 5 dot, coloured by keypoint index (one colour per joint, the same in every detection), for every keypoint whose logit exceeds KP_THRESH (upstream also draws the skeleton's limbs)."""
        H, W = image.shape[:2]
        kps, logits = predictions.get_field("keypoints"), predictions.get_field("keypoint_logits")
        colors = self.compute_colors_for_labels(np.arange(1, kps.shape[1] + 1))
        for k in range(len(predictions)):
            for j in np.nonzero(logits[k] > self.KP_THRESH)[0]:
                x, y = int(kps[k, j, 0]), int(kps[k, j, 1])
                image[max(0, y - 2):min(H, y + 3), max(0, x - 2):min(W, x + 3)] = colors[j]
        return image

    def overlay_class_names(self, image, predictions):
        """demo/predictor.py overlay_class_names: "<class name>: <score>" in white at the top-left corner of every box (README.md:331-334:
        the image run_on_opencv_image returns carries boxes, masks AND labels)."""
        if len(predictions) == 0 or not predictions.has_field("scores"):
            return image
        from PIL import Image, ImageDraw
        pil = Image.fromarray(np.ascontiguousarray(image[:, :, ::-1]))   # BGR -> RGB for PIL
        draw = ImageDraw.Draw(pil)
        scores, labels = predictions.get_field("scores").tolist(), predictions.get_field("labels").tolist()
        for box, score, label in zip(predictions.bbox, scores, labels):
            x, y = int(box[0]), int(box[1])
            draw.text((max(0, x), max(0, y)), "%s: %.2f" % (self.CATEGORIES[int(label)], score), fill=(255, 255, 255))
        image[...] = np.asarray(pil, np.uint8)[:, :, ::-1]
        return image

    def close(self):
        if self._model is not None:
            self._model.close()
            self._model = None


def inference(predictor, images, image_ids=None, batch_size=None, group="canvas", rank=0, world=1, sizes=None, stats=None, force_gather=False,
              workers=4, category_ids=None, resize=None):
    """engine/inference.py-shaped evaluation (README.md:344-347): images -> COCO-format result list (bbox + segm) ready for json.dump.

    The path the benchmark measures, end to end: batches of `batch_size` resized uint8 images go up through pinned memory (double-buffered),
    mean subtraction / padding, the forward, Masker paste at every image's ORIGINAL size, pycocotools RLE and the packing of one fixed-size
    record block all run on the device; the block comes back asynchronously (one rank) or is all-gathered over RCCL (`world` ranks: the
    batches of the global schedule go round-robin to the ranks) while the next batch computes.  Every rank returns the complete
    list, ordered by image, detections in the engine's output order.

    images: sequence of HxWx3 uint8 BGR arrays, or a callable i -> array together with sizes = [(h, w), ...] (lazy loading).
    group:  "canvas" -- batch only images whose padded network canvas is identical, so every image's result equals its single-image
            result (to_image_list pads a batch to its largest member and the RPN sees the padding); "aspect" -- upstream's
            ASPECT_RATIO_GROUPING (portrait / landscape), results then depend on the batch composition exactly as upstream's do.
    stats:  optional dict, receives steps / images / seconds of the device loop.
    workers: host threads that load + resize (PIL, which releases the GIL) the NEXT batch while the current one is enqueued and the previous
            one's records are unpacked; 0 = inline.
    category_ids: the data set's json category id of labels 1, 2, ... (two-stage models; default: the COCO ids for 81 classes, the label itself for
            any other class count).
    A Faster R-CNN predictor (MODEL.MASK_ON False) takes the same loop with the box-only record block: no paste, no RLE, bbox-only results (xywh with
    the legacy +1, no `segmentation` key).  With TEST.BBOX_AUG every step is MaskRCNN.aug_enqueue on the ORIGINAL images -- one rank;
    "canvas" then groups by the canvases of ALL views, so that an image's result still equals its single-image result.  The augmented loop is NOT
    pipelined across steps: every step ends in aug_check (a device synchronisation and the fetch of the pool counters, so that an overflow raises before
    its records are packed); what still overlaps is the worker threads' loading of the next batch, and inside a step the views follow each other as
    consecutive forwards do.
    resize: "host" -- the worker threads resize with PIL and the resized bytes go up; "device" -- the ORIGINAL bytes go up (pinned and staging buffers
            sized by the largest batch's originals) and isegmi_engine_resample_u8 resizes them behind the copy, bit-identical; None: the
            predictor's own setting.  Grouping, canvases and results are the same in both modes."""
    import time
    resize = resize or getattr(predictor, "resize", "host")
    if resize not in ("host", "device"):
        raise ValueError("resize: 'host' or 'device'")
    if getattr(predictor, "is_retinanet", False):
        return _inference_boxes(predictor, images, image_ids, batch_size, group, rank, world, sizes, stats, workers, resize)
    from .coco import label_categories, results_from_records
    from .pipeline import record_capacity, run_record_loop, schedule_batches
    from .transforms import get_size
    from .maskrcnn import padded_canvas
    from . import _ffi
    get = images if callable(images) else images.__getitem__
    if sizes is None:
        if callable(images):
            raise ValueError("inference(): a callable image source needs sizes=[(h, w), ...]")
        sizes = [im.shape[:2] for im in images]
    n_img = len(sizes)
    ids = list(image_ids) if image_ids is not None else list(range(n_img))
    bs = int(batch_size or predictor.max_batch)
    model = predictor.engine(bs)
    cfg = predictor.cfg
    device_resize = resize == "device"
    categories = label_categories(getattr(cfg, "NUM_CLASSES", 81), category_ids)
    box_only = bool(getattr(model, "box_only", False))
    aug = getattr(predictor, "bbox_aug", None)
    if aug is not None and world > 1:
        raise ValueError("inference(): world=%d with TEST.BBOX_AUG.ENABLED -- test-time box augmentation runs on one rank; multi-rank runs are not built for it" % world)
    rs = [get_size(w, h, predictor.min_image_size, predictor.max_image_size) for h, w in sizes]   # resized (h, w) per image
    if group == "canvas" and aug is not None:
        from .maskrcnn import bbox_aug_views
        keys = [tuple(padded_canvas([v[:2]], cfg.SIZE_DIVISIBILITY) for v in bbox_aug_views(hw, cfg, aug, predictor.min_image_size, predictor.max_image_size))
                for hw in sizes]
    elif group == "canvas":
        keys = [padded_canvas([r], cfg.SIZE_DIVISIBILITY) for r in rs]
    elif group == "aspect":
        keys = [int(h >= w) for h, w in sizes]
    else:
        raise ValueError("group: 'canvas' or 'aspect'")
    batches = schedule_batches(keys, bs)
    K = record_capacity(model)
    if aug is not None:   # no pinned input buffers (aug_enqueue uploads the views' bytes itself); the staging holds EVERY size rule's images of a batch
        from .maskrcnn import bbox_aug_views
        area = [sum(v[0] * v[1] * 3 for v in bbox_aug_views(hw, cfg, aug, predictor.min_image_size, predictor.max_image_size) if not v[2]) for hw in sizes]
        pin, stage_bytes = [], max([sum(area[i] for i in b) for b in batches] + [1])
        if device_resize:   # the originals and the tables of every view
            from .maskrcnn import bbox_aug_plan
            stage_bytes = max([bbox_aug_plan([sizes[i] for i in b], cfg, aug, predictor.min_image_size, predictor.max_image_size)[0].nbytes for b in batches] + [1])
    elif device_resize:   # pinned and staging buffers hold the largest batch's ORIGINAL bytes and their tables
        stage_bytes = max([model.original_plan([sizes[i] for i in b], predictor.min_image_size, predictor.max_image_size)[0].nbytes for b in batches] + [1])
        pin = [_ffi.PinnedBuffer((stage_bytes,), np.uint8) for _ in range(2)]
    else:
        pin, stage_bytes = [_ffi.PinnedBuffer((bs * model.H * model.W * 3,), np.uint8) for _ in range(2)], bs * model.H * model.W * 3
    for slot in (0, 1):
        model._u8_staging(slot, stage_bytes)   # device staging at its final size: no sync + re-allocation on a larger batch
    per_image = [None] * n_img

    def consume(step, recs):
        for r, rec in enumerate(recs):       # rank r ran batch step * world + r of the global schedule
            j = step * world + r
            if j >= len(batches):
                continue
            b = batches[j]
            slot_ids = [ids[i] for i in b] + [None] * (bs - len(b))
            slot_hw = [sizes[i] for i in b] + [(1, 1)] * (bs - len(b))
            res = results_from_records(rec, slot_ids, slot_hw, 2, K, categories=categories)
            by_id = {}
            for d in res:
                by_id.setdefault(d["image_id"], []).append(d)
            for i in b:
                per_image[i] = by_id.get(ids[i], [])

    def load(i):   # host: decode + PIL resize (outside the hot path)
        if aug is not None or device_resize:   # the views are resized from the original inside aug_enqueue / on the device
            return get(i)
        return maskrcnn_resize_u8(get(i), predictor.min_image_size, predictor.max_image_size)
    pool = None
    if workers and workers > 0:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=int(workers))
    mine = [j for j in range(rank, len(batches), world)]
    prefetch = {}

    def request(j):
        if j is not None and j < len(batches) and j not in prefetch:
            prefetch[j] = [pool.submit(load, i) for i in batches[j]] if pool else None

    def enqueue(step, slot):
        j = step * world + rank
        if j >= len(batches):
            return False
        b = batches[j]
        request(j + world)                   # the next batch of this rank resizes on the worker threads meanwhile
        futs = prefetch.pop(j, None)         # (a step that is redone after an RLE overflow loads its images again, inline)
        resized = [f.result() for f in futs] if futs else [load(i) for i in b]
        if aug is not None:
            model.aug_enqueue(resized, aug, slot, predictor.min_image_size, predictor.max_image_size, resize)
            model.aug_check()                # BBoxAugOverflow: nothing is truncated silently
            model.set_output_sizes([(w, h) for h, w in (sizes[i] for i in b)])
            return True
        if device_resize:                    # the originals and their tables into pinned memory: one copy, one launch
            plan, hw = model.original_plan([im.shape[:2] for im in resized], predictor.min_image_size, predictor.max_image_size)
            plan.write(pin[slot].array, resized)
            model.upload_original_u8_async(pin[slot], plan, hw, slot)
        else:
            off, hw = 0, []
            for im in resized:               # into pinned memory, back to back
                pin[slot].array[off:off + im.size] = im.reshape(-1)
                off += im.size
                hw.append(im.shape[:2])
            model.upload_u8_async(pin[slot], hw, slot)
        model.forward_device(len(b), slot)
        oh = [sizes[i] for i in b]
        if box_only:   # the record block's one launch scales the boxes to the original sizes
            model.set_output_sizes([(w, h) for h, w in oh])
            return True
        model.paste_device(max(h for h, _ in oh), max(w for _, w in oh), [(w, h) for h, w in oh])
        model.rle_device(oh)
        return True

    t0 = time.perf_counter()
    nsteps = -(-len(batches) // world)
    try:
        if mine:
            request(mine[0])
        # every way out of the loop -- a bad image, an RLE overflow that does not settle, a ctypes error -- restores the engine (whole mask planes
        # again: `sparse_masks`), frees the pinned buffers, stops the worker threads and closes the gather (run_record_loop's own finally)
        run_record_loop(model, bs, nsteps, enqueue, consume, rank, world, force_gather)
    finally:
        if pool:
            pool.shutdown(wait=True, cancel_futures=True)
        for p in pin:
            p.free()
    if stats is not None:
        stats.update(steps=nsteps, images=n_img, seconds=time.perf_counter() - t0, batches=len(batches), batch_size=bs, world=world)
    return [d for r in per_image if r for d in r]


def _inference_boxes(predictor, images, image_ids, batch_size, group, rank, world, sizes, stats, workers, resize="host"):
    """inference() for a detector without masks (RetinaNet): bbox-only COCO results -- xywh with the legacy +1, no `segmentation` key.  Per step the four
    fixed-size detection buffers come back through the engine's two asynchronous download slots into pinned memory; step t's download and step t + 1's
    upload + forward are enqueued before step t's results are unpacked, so the host work hides under the device's."""
    import time
    from .coco import maskrcnn_results
    from .maskrcnn import BoxList, padded_canvas
    from .pipeline import schedule_batches
    from .transforms import get_size
    from . import _ffi
    if world > 1:
        raise ValueError("inference(): world=%d for a RetinaNet predictor -- the gathered record block carries masks; multi-rank runs are not built for this model" % world)
    get = images if callable(images) else images.__getitem__
    if sizes is None:
        if callable(images):
            raise ValueError("inference(): a callable image source needs sizes=[(h, w), ...]")
        sizes = [im.shape[:2] for im in images]
    n_img = len(sizes)
    ids = list(image_ids) if image_ids is not None else list(range(n_img))
    bs = int(batch_size or predictor.max_batch)
    model = predictor.engine(bs)
    cfg = predictor.cfg
    rs = [get_size(w, h, predictor.min_image_size, predictor.max_image_size) for h, w in sizes]
    if group == "canvas":
        keys = [padded_canvas([r], cfg.SIZE_DIVISIBILITY) for r in rs]
    elif group == "aspect":
        keys = [int(h >= w) for h, w in sizes]
    else:
        raise ValueError("group: 'canvas' or 'aspect'")
    batches = schedule_batches(keys, bs)
    device_resize = resize == "device"
    in_bytes = bs * model.H * model.W * 3
    if device_resize:   # the largest batch's ORIGINAL bytes and their tables
        in_bytes = max([model.original_plan([sizes[i] for i in b], predictor.min_image_size, predictor.max_image_size)[0].nbytes for b in batches] + [1])
    pin = [_ffi.PinnedBuffer((in_bytes,), np.uint8) for _ in range(2)]
    out_pin = [_ffi.PinnedBuffer((model.detection_bytes(bs),), np.uint8) for _ in range(2)]
    for slot in (0, 1):
        model._u8_staging(slot, in_bytes)
    per_image = [None] * n_img

    def load(i):
        if device_resize:
            return get(i)
        return maskrcnn_resize_u8(get(i), predictor.min_image_size, predictor.max_image_size)
    pool = None
    if workers and workers > 0:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=int(workers))
    prefetch = {}

    def request(j):
        if j < len(batches) and j not in prefetch:
            prefetch[j] = [pool.submit(load, i) for i in batches[j]] if pool else None

    def enqueue(j):
        slot = j & 1
        b = batches[j]
        request(j + 1)
        futs = prefetch.pop(j, None)
        resized = [f.result() for f in futs] if futs else [load(i) for i in b]
        if device_resize:
            plan, hw = model.original_plan([im.shape[:2] for im in resized], predictor.min_image_size, predictor.max_image_size)
            plan.write(pin[slot].array, resized)
            model.upload_original_u8_async(pin[slot], plan, hw, slot)
        else:
            off, hw = 0, []
            for im in resized:
                pin[slot].array[off:off + im.size] = im.reshape(-1)
                off += im.size
                hw.append(im.shape[:2])
            model.upload_u8_async(pin[slot], hw, slot)
        model.forward_device(len(b), slot)
        model.download_detections_async(slot, out_pin[slot], bs)
        return hw

    def consume(j, hw):
        slot = j & 1
        model.download_wait(slot)
        cnt, box, score, label = model.unpack_detections(out_pin[slot], bs)
        for k, i in enumerate(batches[j]):
            c = int(cnt[k])
            h, w = sizes[i]
            bl = BoxList(box[k, :c], (int(hw[k][1]), int(hw[k][0]))).resize((w, h))
            per_image[i] = maskrcnn_results(ids[i], bl.bbox, score[k, :c], label[k, :c])

    t0 = time.perf_counter()
    try:
        if batches:
            request(0)
        prev = None
        for j in range(len(batches)):
            hw = enqueue(j)
            if prev is not None:
                consume(*prev)
            prev = (j, hw)
        if prev is not None:
            consume(*prev)
        model.sync()
    finally:
        if pool:
            pool.shutdown(wait=True, cancel_futures=True)
        try:
            model.sync()
        finally:
            for p in pin + out_pin:
                p.free()
    if stats is not None:
        stats.update(steps=len(batches), images=n_img, seconds=time.perf_counter() - t0, batches=len(batches), batch_size=bs, world=world)
    return [d for r in per_image if r for d in r]
