"""Command-line front ends shaped like the reference's (README.md:243-249 and README.md:344-347):

  python -m isegmi.cli eval --trained_model=weights.npz --score_threshold=0.15 --top_k=15 --image=in.png[:out.png]
  python -m isegmi.cli eval --trained_model=weights.npz --images=in_dir:out_dir [--output_coco_json=dets.json]
  python -m isegmi.cli test_net --config-file cfg.yaml [--images dir] [--output results.json]
  python -m isegmi.cli pose2seg_test --weights random --anno person_keypoints.json --image-root DIR [--output segm.json] [--batch-size 8]
  python -m isegmi.cli pose2seg_test --weights random --keypoint-config kp.yaml --keypoint-weights random|FILE --anno images.json --image-root DIR
  python -m isegmi.cli yolo_detect --cfg configs/yolov3[-spp|-tiny].cfg --weights random|FILE.npz|FILE.weights --images DIR --output dets.json [--img-size 416] [--pool-pad ignore|zero]
  python -m isegmi.cli vit_classify --model vit_b16 --weights random|FILE.npz --images DIR --topk 5 --output preds.json [--img-size 224] [--num-classes 1000]
  python -m isegmi.cli coco_eval --gt instances.json --dt results.json --iou-type segm|bbox|keypoints [--cat-ids ...] [--max-dets ...] [--out stats.json]

eval, test_net, pose2seg_test and yolo_detect take an optional `--gt instances.json`: after writing their json they print the COCO AP / AR summary.

`--trained_model` / `MODEL.WEIGHT` take the .npz written by tools/import_pth.py; the literal value `random` uses the
seeded synthetic weights (there is no network to fetch the reference's .pth files).  Images are read with PIL.
Both commands run the batched device pipeline (isegmi.predictor.inference / isegmi.yolact.evaluate): uint8 upload, forward, masks at
the original image size, RLE and record packing on the GPU.  Launched as N processes (RANK / LOCAL_RANK / WORLD_SIZE in the environment,
e.g. by `python -m torch.distributed.run --nproc-per-node N -m isegmi.cli ...`) the batches go round-robin to the ranks and the
records are all-gathered with RCCL; rank 0 writes the COCO json.  Nothing here imports torch.
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np


def _load_image_bgr(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1].copy()


def _save_image_bgr(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)


def _weights(spec, kind, depth=50, ycfg=None, gn=False, groups=1, width_per_group=64):
    from .weights import maskrcnn_state_dict, retinanet_state_dict, yolact_state_dict
    if spec in ("", "random", None):
        if kind == "retinanet":
            return retinanet_state_dict(1234, depth, groups=groups, width_per_group=width_per_group)
        if kind == "maskrcnn" and gn:
            return maskrcnn_state_dict(1234, depth, gn=True)
        if kind == "yolact" and ycfg is not None:
            return yolact_state_dict(1234, ycfg.depth, ycfg.num_priors, ycfg.dcn_layers, ycfg.dcn_interval, ycfg.use_maskiou, ycfg.backbone)
        return yolact_state_dict(1234, depth) if kind == "yolact" else maskrcnn_state_dict(1234, depth)
    if not spec.endswith(".npz"):
        raise SystemExit("%s: convert upstream .pth/.pkl with tools/import_pth.py first" % spec)
    return dict(np.load(spec))


def _overlay(img, masks, boxes, classes):
    from .predictor import COCODemo
    colors = COCODemo.compute_colors_for_labels(np.asarray(classes) + 1)
    out = img.copy()
    for k in range(len(classes)):
        m = masks[k].astype(bool)
        out[m] = (0.5 * out[m] + 0.5 * colors[k].astype(np.float32)).astype(np.uint8)
        x1, y1, x2, y2 = (int(v) for v in boxes[k])
        x2, y2 = min(x2, out.shape[1] - 1), min(y2, out.shape[0] - 1)
        out[y1:y2 + 1, [x1, x2]] = colors[k]
        out[[y1, y2], x1:x2 + 1] = colors[k]
    return out


def _rank_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def _image_sizes(files):
    from PIL import Image
    sizes = []
    for f in files:
        with Image.open(f) as im:  # header only
            sizes.append((im.size[1], im.size[0]))
    return sizes


def str2bool(v):
    """upstream eval.py's str2bool: the spelling of its boolean arguments (--fast_nms=False)"""
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def eval_nms_options(a):
    """the suppression-rule arguments of `eval` as YolactConfig fields; an argument not given is upstream's default (fast NMS, per class)"""
    return dict(use_fast_nms=getattr(a, "fast_nms", True), use_cross_class_nms=getattr(a, "cross_class_nms", False),
                nms_trad_cap=getattr(a, "nms_trad_cap", 1024))


def cmd_eval(a):
    """Yolact eval.py: evalimage / evalimages (+ Detections.dump when --output_coco_json is given)."""
    from .coco import dump, rle_decode
    from .yolact import Yolact, YolactConfig, evaluate
    refuse_device_resize(a, "Yolact", "isegmi_op_preprocess_u8 resizes to the square canvas on the device")
    # upstream eval.py --config: yolact_resnet50_config (default here), yolact_base_config (R101), yolact_im700_config, and the
    # YOLACT++ pair yolact_plus_resnet50_config / yolact_plus_base_config (DCNv2 backbones, 9 anchors, mask re-scoring)
    cfg = {"yolact_resnet50_config": YolactConfig(), "yolact_base_config": YolactConfig.base(), "yolact_im700_config": YolactConfig.im700(),
           "yolact_plus_resnet50_config": YolactConfig.plus_resnet50(), "yolact_plus_base_config": YolactConfig.plus_base(),
           "yolact_darknet53_config": YolactConfig.darknet53()}[a.config]
    # upstream eval.py --fast_nms / --cross_class_nms (set_cfg: cfg.use_fast_nms / cfg.use_cross_class_nms); --nms_trad_cap is this engine's
    cfg = dataclasses.replace(cfg, **eval_nms_options(a))
    rank, world, local = _rank_world()
    jobs = []
    if a.image:
        src, _, dst = a.image.partition(":")
        jobs.append((src, dst or None))
    if a.images:
        src, _, dst = a.images.partition(":")
        os.makedirs(dst, exist_ok=True)
        for f in sorted(os.listdir(src)):
            jobs.append((os.path.join(src, f), os.path.join(dst, os.path.splitext(f)[0] + ".png")))
    files = [j[0] for j in jobs]
    sizes = _image_sizes(files)
    net = Yolact(_weights(a.trained_model, "yolact", cfg.depth, cfg), cfg, max_batch=a.batch_size, device=local)
    results = evaluate(net, lambda i: _load_image_bgr(files[i]), batch_size=a.batch_size, score_threshold=a.score_threshold, top_k=a.top_k,
                       rank=rank, world=world, sizes=sizes)
    painted = {}
    if getattr(a, "render", "host") == "device" and rank == 0:   # --render=device: the outputs are painted from the mask planes, on the device
        from .yolact import render_images
        todo = [i for i, (_, dst) in enumerate(jobs) if dst]
        painted = dict(zip(todo, render_images(net, [_load_image_bgr(files[i]) for i in todo], a.score_threshold, a.top_k, a.batch_size)))
    net.close()
    if rank == 0:
        by_img = {}
        for r in results:
            by_img.setdefault(r["image_id"], []).append(r)
        for i, (src, dst) in enumerate(jobs):
            dets = by_img.get(i, [])
            print("%s: %d detections" % (src, len(dets)))
            if i in painted:
                _save_image_bgr(dst, painted[i])
            elif dst and dets:  # overlay from the records themselves: RLE -> mask, xywh -> box
                from .coco import COCO_CATEGORY_IDS
                masks = np.stack([rle_decode(d["segmentation"]) for d in dets])
                boxes = [[d["bbox"][0], d["bbox"][1], d["bbox"][0] + d["bbox"][2], d["bbox"][1] + d["bbox"][3]] for d in dets]
                classes = [COCO_CATEGORY_IDS.index(d["category_id"]) for d in dets]
                _save_image_bgr(dst, _overlay(_load_image_bgr(src), masks, boxes, classes))
            elif dst:
                _save_image_bgr(dst, _load_image_bgr(src))
        if a.output_coco_json:
            dump(results, a.output_coco_json)
        if a.gt:
            _print_coco_summary(a.gt, results, ("bbox", "segm"))
    return results


def refuse_device_resize(a, model, why):
    """--resize device on a command whose model keeps its own front end: refused by name."""
    if getattr(a, "resize", "host") == "device":
        raise SystemExit("--resize device: %s keeps its own front end (%s); the PIL-exact device resize is built for the R-CNN family, RetinaNet and YOLOv3" % (model, why))


def cmd_test_net(a):
    """tools/test_net.py: build the model from the yaml, run inference() over the images, write COCO-format json."""
    from .config import cfg, is_bbox_aug, is_keypoint_rcnn, is_retinanet, to_bbox_aug_config, to_keypointrcnn_config, to_maskrcnn_config, to_retinanet_config
    from .predictor import COCODemo, inference
    c = cfg.clone()
    if a.config_file:
        c.merge_from_file(a.config_file)
    c.merge_from_list(a.opts)
    retina = is_retinanet(c)   # MODEL.RETINANET_ON: the one-stage detector, bbox results only
    # TEST.BBOX_AUG.ENABLED: multi-scale + flip inference of a box-only model; the other mappings refuse the key by name
    bbox_aug = None
    if is_bbox_aug(c) and not retina and not is_keypoint_rcnn(c):
        mc_aug, bbox_aug = to_bbox_aug_config(c)
    # MODEL.KEYPOINT_ON: Keypoint R-CNN -- one json entry per detection with `keypoints`; --gt prints the bbox block and then the keypoints block
    mc = mc_aug if bbox_aug is not None else to_retinanet_config(c) if retina else to_keypointrcnn_config(c) if is_keypoint_rcnn(c) else to_maskrcnn_config(c)
    rank, world, local = _rank_world()
    files = sorted(os.path.join(a.images, f) for f in os.listdir(a.images)) if a.images else []
    if retina:
        sd = _weights(c.MODEL.WEIGHT, "retinanet", mc.depth, groups=mc.NUM_GROUPS, width_per_group=mc.WIDTH_PER_GROUP)
    elif c.MODEL.WEIGHT in ("", "random", None):   # the seeded generator of the configured model: body, norm, MASK_ON, NUM_CLASSES, CLS_AGNOSTIC_BBOX_REG
        from .weights import random_maskrcnn_state_dict
        sd = random_maskrcnn_state_dict(mc, 1234)
    else:
        sd = _weights(c.MODEL.WEIGHT, "maskrcnn", mc.depth, gn=mc.USE_GN)
    box_only = retina or not mc.MASK_ON   # RetinaNet and Faster R-CNN (MODEL.MASK_ON False): bbox results only
    demo = COCODemo(mc, min_image_size=mc.MIN_SIZE_TEST, confidence_threshold=0.0, state_dict=sd,
                    max_image_size=mc.MAX_SIZE_TEST, device=local, max_batch=a.batch_size, bbox_aug=bbox_aug, resize=getattr(a, "resize", "host"))
    stats = {}
    results = inference(demo, lambda i: _load_image_bgr(files[i]), batch_size=a.batch_size, group=a.group, rank=rank, world=world,
                        sizes=_image_sizes(files), stats=stats) if files else []
    vis_dir = getattr(a, "vis_dir", None)
    if vis_dir and rank == 0:   # the Detectron example's last line for every image: run_on_opencv_image -> an annotated file
        os.makedirs(vis_dir, exist_ok=True)
        demo.confidence_threshold, demo.render = getattr(a, "vis_threshold", 0.7), getattr(a, "render", "host")
        for f in files:
            _save_image_bgr(os.path.join(vis_dir, os.path.splitext(os.path.basename(f))[0] + ".png"), demo.run_on_opencv_image(_load_image_bgr(f)))
    demo.close()
    if rank == 0:
        with open(a.output, "w") as f:
            json.dump(results, f)
        print("wrote %d results for %d images to %s (%d steps of %d images on %d rank(s))" % (
            len(results), len(files), a.output, stats.get("steps", 0), a.batch_size, world))
        if a.gt:
            _print_coco_summary(a.gt, results, ("bbox", "keypoints") if is_keypoint_rcnn(c) else ("bbox",) if box_only else ("bbox", "segm"))
    return results


def cmd_pose2seg_test(a):
    """Pose2Seg test.py (README section 2.2): images + COCO person keypoints -> COCO segmentation json (category 1, score 1.0)."""
    from .pose2seg import Pose2Seg, Pose2SegConfig, read_person_keypoints, test
    refuse_device_resize(a, "Pose2Seg", "its affine letterbox, isegmi_op_pose2seg_letterbox, already runs on the device")
    from .weights import pose2seg_state_dict
    if a.weights in ("", "random", None):
        sd = pose2seg_state_dict(1234)
    elif a.weights.endswith(".npz"):
        sd = dict(np.load(a.weights))
    else:
        raise SystemExit("%s: Pose2Seg takes .npz weights in this engine's names (importing last.pkl is out of scope)" % a.weights)
    _, _, local = _rank_world()
    if hasattr(a, "keypoint_config") or hasattr(a, "keypoint_weights"):
        return _pose2seg_from_detector(a, sd, local)
    images, kps = read_person_keypoints(a.anno)
    images = [im for im in images if im["id"] in kps]
    net = Pose2Seg(sd, Pose2SegConfig(), max_batch=a.batch_size, max_instances=a.max_instances, device=local)
    results = test(net, lambda i: _load_image_bgr(os.path.join(a.image_root, images[i]["file_name"])), [kps[im["id"]] for im in images],
                   [im["id"] for im in images], batch_size=a.batch_size)
    net.close()
    with open(a.output, "w") as f:
        json.dump(results, f)
    print("wrote %d person masks for %d images to %s" % (len(results), len(images), a.output))
    if a.gt:
        _print_coco_summary(a.gt, results, ("segm",))
    return results


def _pose2seg_from_detector(a, sd, local):
    """pose2seg_test with --keypoint-config / --keypoint-weights: --anno supplies only the image list, a Keypoint R-CNN finds the persons and their
    keypoints; every entry's score is the detection's box score."""
    from .config import cfg, is_keypoint_rcnn, to_keypointrcnn_config
    from .maskrcnn import MaskRCNN
    from .pose2seg import KeypointPose2Seg, Pose2Seg, Pose2SegConfig, test_from_images
    if not getattr(a, "keypoint_config", None):
        raise SystemExit("--keypoint-weights needs --keypoint-config YAML (the Keypoint R-CNN's config)")
    c = cfg.clone()
    c.merge_from_file(a.keypoint_config)
    c.merge_from_list(getattr(a, "keypoint_opts", []))
    if not is_keypoint_rcnn(c):
        raise SystemExit("%s: MODEL.KEYPOINT_ON is False; --keypoint-config takes a Keypoint R-CNN config" % a.keypoint_config)
    mc = to_keypointrcnn_config(c)
    spec = getattr(a, "keypoint_weights", "random") or "random"
    if spec == "random":
        from .weights import random_maskrcnn_state_dict
        ksd = random_maskrcnn_state_dict(mc, 1234)
    elif spec.endswith(".npz"):
        ksd = dict(np.load(spec))
    else:
        raise SystemExit("%s: convert upstream .pth/.pkl with tools/import_pth.py first" % spec)
    with open(a.anno) as f:
        images = list(json.load(f).get("images", []))
    d = mc.SIZE_DIVISIBILITY
    side = -(-max(mc.MIN_SIZE_TEST, mc.MAX_SIZE_TEST) // d) * d
    det = MaskRCNN(ksd, side, side, cfg=mc, max_batch=a.batch_size, device=local)
    net = Pose2Seg(sd, Pose2SegConfig(), max_batch=a.batch_size, max_instances=a.max_instances, device=local)
    pipe = KeypointPose2Seg(det, net, person_threshold=getattr(a, "person_threshold", 0.5), keypoint_threshold=getattr(a, "keypoint_threshold", 2.0))
    try:
        results = test_from_images(pipe, lambda i: _load_image_bgr(os.path.join(a.image_root, images[i]["file_name"])), [im["id"] for im in images],
                                   batch_size=a.batch_size)
    finally:
        pipe.close()
        net.close()
        det.close()
    with open(a.output, "w") as f:
        json.dump(results, f)
    print("wrote %d person masks for %d images to %s (persons from the keypoint detector)" % (len(results), len(images), a.output))
    if a.gt:
        _print_coco_summary(a.gt, results, ("segm",))
    return results


def yolo_config(a):
    """The YoloV3Config of a yolo_detect command line: the .cfg's model, the canvas of --img-size, the thresholds given."""
    from .config import parse_darknet_cfg
    kw = {}
    if a.conf_thres is not None:
        kw["conf_thresh"] = a.conf_thres
    if a.nms_thres is not None:
        kw["nms_thresh"] = a.nms_thres
    if a.bn_eps is not None:
        kw["bn_eps"] = a.bn_eps
    if a.best_class:
        kw["multi_label"] = False
    if a.pool_pad is not None:
        kw["pool_pad"] = a.pool_pad
    with open(a.cfg) as f:
        ycfg = parse_darknet_cfg(f.read(), **kw)
    if a.img_size:
        import dataclasses
        hw = a.img_size if len(a.img_size) == 2 else a.img_size * 2
        ycfg = dataclasses.replace(ycfg, height=hw[0], width=hw[1]).validate()
    return ycfg


def cmd_yolo_detect(a):
    """YOLOv3 detect / test: letterbox, forward, boxes back in image coordinates -> bbox-only COCO json (xywh, plain widths)."""
    from .coco import dump, label_categories, yolo_results
    from .weights import load_darknet_weights, yolov3_state_dict
    from .yolov3 import YoloDetector
    _, world, local = _rank_world()
    if world > 1:
        raise SystemExit("yolo_detect: WORLD_SIZE=%d: multi-rank inference (world > 1) is not built for YOLOv3" % world)
    ycfg = yolo_config(a)
    if a.weights in ("", "random", None):
        sd = yolov3_state_dict(1234, ycfg.classes, ycfg.variant)
    elif a.weights.endswith(".npz"):
        sd = dict(np.load(a.weights))
    elif a.weights.endswith(".weights"):
        sd = load_darknet_weights(a.weights, ycfg)
    else:
        raise SystemExit("%s: --weights takes random, an .npz in this engine's names or a darknet .weights file" % a.weights)
    files = sorted(os.path.join(a.images, f) for f in os.listdir(a.images))
    cats = label_categories(ycfg.classes + 1)
    det = YoloDetector(sd, ycfg, max_batch=a.batch_size, device=local, resize=getattr(a, "resize", "host"))
    results = []
    try:
        for i0 in range(0, len(files), a.batch_size):
            dets = det.detect([_load_image_bgr(f) for f in files[i0:i0 + a.batch_size]])
            for k, (boxes, scores, labels) in enumerate(dets):
                results += yolo_results(i0 + k, boxes, scores, labels, cats)
    finally:
        det.close()
    dump(results, a.output)
    print("wrote %d detections for %d images to %s" % (len(results), len(files), a.output))
    if a.gt:
        _print_coco_summary(a.gt, results, ("bbox",))
    return results


def vit_config(a):
    """The ViTConfig of a vit_classify command line."""
    from .vit import ViTConfig
    return ViTConfig.named(a.model, num_classes=a.num_classes, topk=a.topk, gelu_tanh=bool(a.gelu_tanh), ln_eps=a.ln_eps).validate(a.img_size, a.img_size)


def cmd_vit_classify(a):
    """ViT classification over a directory of images -> json: one entry per image with its top-k labels and probabilities."""
    from .vit import ViTClassifier
    refuse_device_resize(a, "ViT", "isegmi_op_preprocess_u8 resizes to the square canvas on the device")
    from .weights import vit_random_state_dict
    _, world, local = _rank_world()
    if world > 1:
        raise SystemExit("vit_classify: WORLD_SIZE=%d: multi-rank inference (world > 1) is not built for ViT" % world)
    cfg = vit_config(a)
    if a.weights in ("", "random", None):
        sd = vit_random_state_dict(cfg, 1234, a.img_size, a.img_size)
    elif a.weights.endswith(".npz"):
        sd = dict(np.load(a.weights))
    else:
        raise SystemExit("%s: --weights takes random or an .npz in the timm names (tools/import_pth.py --family %s writes one)" % (a.weights, a.model))
    files = sorted(os.path.join(a.images, f) for f in os.listdir(a.images))
    clf = ViTClassifier(sd, cfg, a.img_size, a.img_size, max_batch=a.batch_size, device=local)
    results = []
    try:
        for i0 in range(0, len(files), a.batch_size):
            chunk = files[i0:i0 + a.batch_size]
            for f, (labels, probs) in zip(chunk, clf.classify([_load_image_bgr(f) for f in chunk])):
                results.append({"file": os.path.basename(f), "labels": [int(v) for v in labels], "probabilities": [float(v) for v in probs]})
    finally:
        clf.close()
    with open(a.output, "w") as f:
        json.dump(results, f)
    print("wrote the top-%d classes of %d images to %s" % (cfg.topk, len(files), a.output))
    return results


def _print_coco_summary(gt_path, results, iou_types, cat_ids=None, max_dets=None):
    """The COCO summary of a result list against an annotation file, as the reference's test commands print it."""
    from .cocoeval import evaluate_results
    if not results:
        print("no results to evaluate")
        return {}
    return evaluate_results(gt_path, results, iou_types, cat_ids=cat_ids, max_dets=max_dets, verbose=True)


def cmd_coco_eval(a):
    stats = _print_coco_summary(a.gt, a.dt, (a.iou_type,), a.cat_ids, a.max_dets)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({k: [float(x) for x in v] for k, v in stats.items()}, f)
    return stats


def build_parser():
    ap = argparse.ArgumentParser(prog="isegmi.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("eval", help="Yolact eval.py-style image evaluation")
    e.add_argument("--trained_model", default="random")
    e.add_argument("--config", default="yolact_resnet50_config", choices=["yolact_resnet50_config", "yolact_base_config", "yolact_im700_config", "yolact_plus_resnet50_config", "yolact_plus_base_config", "yolact_darknet53_config"])
    e.add_argument("--score_threshold", type=float, default=0.0)
    e.add_argument("--top_k", type=int, default=5)
    e.add_argument("--image", default=None, help="in.png[:out.png]")
    e.add_argument("--images", default=None, help="in_dir:out_dir")
    e.add_argument("--output_coco_json", default=None)
    e.add_argument("--batch_size", type=int, default=8, help="images per step and rank")
    e.add_argument("--render", default=argparse.SUPPRESS, choices=["host", "device"],
                   help="(default host) the --image / --images outputs: host draws them from the decoded records, device paints them from the mask planes (isegmi.yolact.render_images)")
    e.add_argument("--resize", default=argparse.SUPPRESS, choices=["host", "device"], help="refused for Yolact: its front end already resizes on the device")
    e.add_argument("--fast_nms", type=str2bool, default=argparse.SUPPRESS, help="(default True) False: traditional per-class NMS (upstream's cython_nms) instead of fast NMS")
    e.add_argument("--cross_class_nms", type=str2bool, default=argparse.SUPPRESS, help="(default False) True: one fast-NMS pass over all classes together")
    e.add_argument("--nms_trad_cap", type=int, default=argparse.SUPPRESS, help="(default 1024) traditional NMS: candidates visited per image and class (a multiple of 64 in [64, 2048])")
    t = sub.add_parser("test_net", help="detectron tools/test_net.py-style evaluation -> COCO json")
    t.add_argument("--config-file", dest="config_file", default="")
    t.add_argument("--images", default=None, help="directory of images (the COCO dataset catalog is out of scope)")
    t.add_argument("--output", default="results.json")
    t.add_argument("--batch_size", type=int, default=2, help="images per step and rank (TEST.IMS_PER_BATCH / ranks)")
    t.add_argument("--group", default="canvas", choices=["canvas", "aspect"],
                   help="canvas: batch only images with the same padded canvas (every result equals the single-image result); aspect: upstream's ASPECT_RATIO_GROUPING")
    # like the detector flags of pose2seg_test, these leave no attribute behind unless given
    t.add_argument("--vis-dir", dest="vis_dir", default=argparse.SUPPRESS, help="also write COCODemo.run_on_opencv_image of every image (masks, boxes, names) to this directory")
    t.add_argument("--vis-threshold", dest="vis_threshold", type=float, default=argparse.SUPPRESS, help="(default 0.7) with --vis-dir: draw detections with score > this")
    t.add_argument("--render", default=argparse.SUPPRESS, choices=["host", "device"], help="(default host) with --vis-dir: where the masks, boxes and dots are drawn (DESIGN.md 22)")
    t.add_argument("--resize", default=argparse.SUPPRESS, choices=["host", "device"],
                   help="(default host) where the test-time resize runs: host = PIL on worker threads, device = the original bytes go up and one kernel resizes them, bit-identical (DESIGN.md 24)")
    t.add_argument("opts", nargs=argparse.REMAINDER, default=[])
    p = sub.add_parser("pose2seg_test", help="Pose2Seg test.py-style evaluation: images + COCO person keypoints -> COCO segmentation json")
    p.add_argument("--weights", default="random", help="random (seeded synthetic weights) or an .npz in this engine's names")
    p.add_argument("--anno", required=True, help="COCO person_keypoints json")
    p.add_argument("--image-root", dest="image_root", required=True)
    p.add_argument("--output", default="segm.json")
    p.add_argument("--batch-size", dest="batch_size", type=int, default=8)
    p.add_argument("--resize", default=argparse.SUPPRESS, choices=["host", "device"], help="refused for Pose2Seg: its letterbox already runs on the device")
    p.add_argument("--max-instances", dest="max_instances", type=int, default=32)
    # the detector flags leave no attribute behind unless given: without them the command is the one it was
    p.add_argument("--keypoint-config", dest="keypoint_config", default=argparse.SUPPRESS,
                   help="Keypoint R-CNN yaml: the persons and their keypoints come from this detector, --anno then supplies only the image list")
    p.add_argument("--keypoint-weights", dest="keypoint_weights", default=argparse.SUPPRESS, help="random or FILE (.npz) for the detector of --keypoint-config")
    p.add_argument("--keypoint-opts", dest="keypoint_opts", nargs="*", default=argparse.SUPPRESS, help="KEY VALUE pairs merged into the detector's config, as test_net's opts")
    p.add_argument("--person-threshold", dest="person_threshold", type=float, default=argparse.SUPPRESS, help="with --keypoint-config: keep detections with score > this")
    p.add_argument("--keypoint-threshold", dest="keypoint_threshold", type=float, default=argparse.SUPPRESS,
                   help="with --keypoint-config: a keypoint is visible where its logit > this")
    y = sub.add_parser("yolo_detect", help="YOLOv3 detection over a directory of images -> bbox-only COCO json")
    y.add_argument("--cfg", default="configs/yolov3.cfg", help="darknet yolov3.cfg, yolov3-spp.cfg or yolov3-tiny.cfg (these three topologies are built)")
    y.add_argument("--weights", default="random", help="random (seeded synthetic weights), FILE.npz in this engine's names, or a darknet FILE.weights")
    y.add_argument("--images", required=True, help="directory of images; image_id = index in sorted order")
    y.add_argument("--img-size", dest="img_size", type=int, nargs="+", default=None, help="canvas side, or height and width (multiples of 32 in 32..1024; default: the cfg's)")
    y.add_argument("--conf-thres", dest="conf_thres", type=float, default=None, help="objectness x class score threshold (default 0.5)")
    y.add_argument("--nms-thres", dest="nms_thres", type=float, default=None, help="class-wise NMS IoU threshold (default 0.4)")
    y.add_argument("--bn-eps", dest="bn_eps", type=float, default=None, help="BatchNorm epsilon of the fold: 1e-5 (default) or darknet's 1e-6")
    y.add_argument("--best-class", dest="best_class", action="store_true", help="one candidate per anchor, its best class, instead of every class over the threshold")
    y.add_argument("--pool-pad", dest="pool_pad", choices=["ignore", "zero"], default=None,
                   help="yolov3-spp / -tiny max-pools: a tap outside the map is skipped (ignore: darknet, default) or counts as 0 (zero: the PyTorch ports)")
    y.add_argument("--resize", default=argparse.SUPPRESS, choices=["host", "device"],
                   help="(default host) where the letterbox runs: host = PIL, device = the original bytes go up and one kernel makes the canvas, bit-identical (DESIGN.md 24)")
    y.add_argument("--output", default="dets.json")
    y.add_argument("--batch-size", dest="batch_size", type=int, default=8)
    for q in (e, t, p, y):
        q.add_argument("--gt", default=None, help="COCO annotation json: print the COCO AP / AR summary of the written results (isegmi.cocoeval)")
    v = sub.add_parser("vit_classify", help="ViT classification over a directory of images -> json of top-k labels and probabilities")
    v.add_argument("--model", default="vit_b16", choices=["vit_ti16", "vit_s16", "vit_b16", "vit_b32", "vit_l16"])
    v.add_argument("--weights", default="random", help="random (seeded synthetic weights) or FILE.npz in the timm names")
    v.add_argument("--images", required=True, help="directory of images, classified in sorted order")
    v.add_argument("--topk", type=int, default=5)
    v.add_argument("--num-classes", dest="num_classes", type=int, default=1000)
    v.add_argument("--img-size", dest="img_size", type=int, default=224, help="canvas side: a multiple of the patch size; the position embedding is not interpolated")
    v.add_argument("--gelu-tanh", dest="gelu_tanh", type=int, default=0, choices=[0, 1], help="1: the tanh GELU of the original JAX release")
    v.add_argument("--ln-eps", dest="ln_eps", type=float, default=1e-6)
    v.add_argument("--resize", default=argparse.SUPPRESS, choices=["host", "device"], help="refused for ViT: its front end already resizes on the device")
    v.add_argument("--output", default="preds.json")
    v.add_argument("--batch-size", dest="batch_size", type=int, default=8)
    c = sub.add_parser("coco_eval", help="COCO AP / AR of a result json against an annotation json (pycocotools COCOeval restated)")
    c.add_argument("--gt", required=True, help="COCO annotation json")
    c.add_argument("--dt", required=True, help="COCO result json")
    c.add_argument("--iou-type", dest="iou_type", default="segm", choices=["segm", "bbox", "keypoints"])
    c.add_argument("--cat-ids", dest="cat_ids", type=int, nargs="+", default=None)
    c.add_argument("--max-dets", dest="max_dets", type=int, nargs="+", default=None)
    c.add_argument("--out", default=None, help="also write the stats (twelve; ten for keypoints) as json")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    return {"eval": cmd_eval, "test_net": cmd_test_net, "pose2seg_test": cmd_pose2seg_test, "yolo_detect": cmd_yolo_detect,
            "vit_classify": cmd_vit_classify, "coco_eval": cmd_coco_eval}[a.cmd](a)


if __name__ == "__main__":
    main()
