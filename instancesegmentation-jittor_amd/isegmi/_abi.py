"""The C ABI of libisegmi.so as ctypes sees it, said once: every function of include/isegmi.h with its restype and argtypes, and every
ctypes.Structure that mirrors one of the header's structs.  _ffi.lib() applies SIGNATURES right after loading the library, so a call with
the wrong arity or a float where an integer belongs raises in Python instead of shifting arguments into a kernel.

One mechanical rule maps the header to the table (tests/test_abi_cpu.py parses the header and holds the table to it, both ways):
    int, int32_t -> c_int      int64_t -> c_int64      float -> c_float      double -> c_double
    const char* (parameter or return) -> c_char_p      every other pointer (void*, T*, T**, struct pointers, handles, streams) -> c_void_p
c_void_p takes None, Python ints, c_void_p, byref(...), ctypes arrays and buffers, bytes and .ctypes.data_as(c_void_p); a numpy integer
used as an address needs int(...).  c_int / c_int64 take numpy integers and bools and refuse floats.
"""
import ctypes as C

RETINA_MAX_LEVELS = 5   # ISEGMI_RETINA_MAX_LEVELS


def _i32(*names):
    return [(n, C.c_int32) for n in names]


def _ptr(*names):
    return [(n, C.c_void_p) for n in names]


class ConvDesc(C.Structure):
    """isegmi_conv_desc"""
    _fields_ = _i32("N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "act", "tile", "out_div") + \
        [("out_img_stride", C.c_int64), ("out_pix_stride", C.c_int64)]


class BottleneckDesc(C.Structure):
    """isegmi_bottleneck_desc"""
    _fields_ = _i32("N", "H", "W", "Cin", "Cmid", "flags")


class YolactDetectArgs(C.Structure):
    """isegmi_yolact_detect_args"""
    _fields_ = _i32("N", "P", "ncls", "mask_dim", "top_k", "max_det") + [("conf_thresh", C.c_float), ("nms_thresh", C.c_float)] + \
        _ptr("d_conf", "d_loc", "d_mask", "d_priors", "d_ws_scoresT", "d_ws_boxes", "d_ws_counts", "d_ws_tk_vals", "d_ws_tk_idx", "d_ws_tk_cnt",
             "d_ws_cand", "d_ws_fin_vals", "d_ws_fin_idx", "d_ws_fin_cnt", "d_out_count", "d_out_boxes", "d_out_scores", "d_out_classes",
             "d_out_coeffs", "d_out_prior") + \
        _i32("A", "mask_tanh") + [("pix_stride", C.c_int64)] + _i32("off_loc", "off_conf", "off_mask", "second_threshold") + \
        _i32("nms_mode", "trad_cap") + [("trad_scale", C.c_float)] + \
        _ptr("d_out_nms_total", "d_out_nms_overflow", "d_ws_cc_scores", "d_ws_cc_class", "d_ws_trad_list", "d_ws_trad_prior")


class BoxPostArgs(C.Structure):
    """isegmi_box_post_args"""
    _fields_ = _i32("N", "R", "ncls", "det_per_img", "cap", "nms_flags") + \
        [("score_thresh", C.c_float), ("nms_thresh", C.c_float), ("logits_stride", C.c_int64), ("regr_stride", C.c_int64)] + \
        _ptr("d_logits", "d_regr", "d_props", "d_prop_cnt", "d_image_hw", "d_ws_prob", "d_ws_cand_scores", "d_ws_cand_boxes", "d_ws_kept_total",
             "d_ws_top_vals", "d_ws_top_idx", "d_out_count", "d_out_boxes", "d_out_scores", "d_out_labels", "d_ws_crowd_matrix", "d_ws_crowd_keys",
             "d_ws_crowd_boxes", "d_ws_crowd_m") + \
        _i32("cls_agnostic")


class RetinaSelectArgs(C.Structure):
    """isegmi_retina_select_args"""
    _fields_ = _i32("nl", "N", "A", "C", "top_n") + [("score_thresh", C.c_float), ("min_size", C.c_float), ("HW", C.c_int32 * RETINA_MAX_LEVELS),
                                                     ("d_logits", C.c_void_p * RETINA_MAX_LEVELS), ("d_deltas", C.c_void_p * RETINA_MAX_LEVELS),
                                                     ("d_anchors", C.c_void_p * RETINA_MAX_LEVELS), ("d_image_hw", C.c_void_p), ("d_ws", C.c_void_p),
                                                     ("ws_bytes", C.c_int64)] + \
        _ptr("d_sel_scores", "d_sel_idx", "d_sel_cnt", "d_out_boxes", "d_out_scores", "d_out_labels", "d_out_cnt")


class RetinaPostArgs(C.Structure):
    """isegmi_retina_post_args"""
    _fields_ = _i32("N", "nseg", "seg_len", "ncls", "det_per_img", "cap", "nms_flags") + [("nms_thresh", C.c_float)] + \
        _ptr("d_boxes", "d_scores", "d_labels", "d_seg_cnt", "d_ws") + [("ws_bytes", C.c_int64)] + \
        _ptr("d_out_count", "d_out_boxes", "d_out_scores", "d_out_labels")


class RleArgs(C.Structure):
    """isegmi_rle_args"""
    _fields_ = _i32("N", "K", "plane_h", "plane_w", "cap_runs", "cap_chars") + \
        _ptr("d_masks", "d_count", "d_image_hw", "d_windows", "d_ws_trans", "d_ws_col", "d_ws_nruns", "d_ws_tile", "d_ws_len", "d_ws_starts",
             "d_out_run_off", "d_out_counts", "d_out_str_off", "d_out_chars", "d_out_status")


class P2sImage(C.Structure):
    """isegmi_p2s_image: one image of a letterbox batch."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("minv", C.c_float * 6), ("reserved", C.c_int32 * 2)]


class CocoMatchArgs(C.Structure):
    """isegmi_coco_match_args"""
    _fields_ = _i32("n_groups", "A", "T", "reserved") + [("n_dets", C.c_int64), ("n_gts", C.c_int64), ("n_ious", C.c_int64)] + \
        _ptr("d_det_off", "d_gt_off", "d_iou_off", "d_ious", "d_det_area", "d_gt_area", "d_gt_crowd", "d_gt_ignore", "d_area_rng", "d_iou_thrs",
             "d_dt_match", "d_dt_ignore", "d_gt_match", "d_gt_ignore_out")


STRUCTS = {"isegmi_conv_desc": ConvDesc, "isegmi_bottleneck_desc": BottleneckDesc, "isegmi_yolact_detect_args": YolactDetectArgs,
           "isegmi_box_post_args": BoxPostArgs, "isegmi_retina_select_args": RetinaSelectArgs, "isegmi_retina_post_args": RetinaPostArgs,
           "isegmi_rle_args": RleArgs, "isegmi_p2s_image": P2sImage, "isegmi_coco_match_args": CocoMatchArgs}

I, L, F, D, S, V = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p, C.c_void_p

# name: (restype, [argtypes]), in the header's order
SIGNATURES = {
    "isegmi_version": (I, []),
    "isegmi_last_error": (S, []),
    "isegmi_device_count": (I, [V]),
    "isegmi_set_device": (I, [I]),
    "isegmi_malloc": (I, [V, L]),
    "isegmi_free": (I, [V]),
    "isegmi_malloc_host": (I, [V, L]),
    "isegmi_free_host": (I, [V]),
    "isegmi_h2d": (I, [V, V, L]),
    "isegmi_d2h": (I, [V, V, L]),
    "isegmi_memset": (I, [V, I, L]),
    "isegmi_sync": (I, []),
    "isegmi_box_calibrate": (I, [D, V, V, V]),
    "isegmi_conv_out_hw": (I, [V, V, V]),
    "isegmi_conv_split_qualifies": (I, [V]),
    "isegmi_conv_packed_floats": (I, [V, V]),
    "isegmi_pack_conv_weights": (I, [V, V, V]),
    "isegmi_op_conv2d": (I, [V, V, V, V, V, V, V, V]),
    "isegmi_op_conv2d_group": (I, [I, V, V, V, V, V, V, V, V]),
    "isegmi_conv_grouped_packed_floats": (I, [V, I, V]),
    "isegmi_pack_conv_weights_grouped": (I, [V, I, V, V]),
    "isegmi_op_conv2d_grouped": (I, [V, I, V, V, V, V, V, V, V]),
    "isegmi_conv_packed_halfs": (I, [V, V]),
    "isegmi_pack_conv_weights_f16": (I, [V, V, V]),
    "isegmi_op_conv2d_f16": (I, [V, V, V, V, V, V, V, I, V]),
    "isegmi_op_bottleneck_f16": (I, [V, V, V, V, V, V, V, V, V, V, V, V, V]),
    "isegmi_op_bottleneck_ds_f16": (I, [V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V]),
    "isegmi_op_conv1x1_up2x_add_f16": (I, [V, V, V, V, V, V, I, I, V, V]),
    "isegmi_op_conv3x3_head_f16": (I, [V, V, V, V, V, V, V, V, I, V, V, V]),
    "isegmi_op_pad_c3_to_f16_halo": (I, [V, I, I, I, V, V]),
    "isegmi_op_stem_pool_f16": (I, [I, I, I, V, V, V, V, V, I, V]),
    "isegmi_set_f16_mfma_shape": (I, [I]),
    "isegmi_get_f16_mfma_shape": (I, [V]),
    "isegmi_op_preprocess_u8": (I, [V, I, I, I, V, I, I, I, I, L, V, V, I, V]),
    "isegmi_op_preprocess_u8_flip": (I, [V, I, I, I, V, I, I, I, I, L, V, V, I, I, V]),
    "isegmi_resample_coeffs": (I, [I, I, V, V, V]),
    "isegmi_op_resample_u8": (I, [V, L, V, V, I, V, L, V, I, I, I, L, V, V, I, F, V, L, V]),
    "isegmi_op_resample_tile": (I, [V, V, V]),
    "isegmi_op_maxpool": (I, [V, I, I, I, I, I, I, I, V, V]),
    "isegmi_op_resize_bilinear": (I, [V, I, I, I, I, I, I, V, I, V, V]),
    "isegmi_op_keypoint_heatmap": (I, [V, L, I, I, I, V, V]),
    "isegmi_op_keypoint_decode": (I, [V, V, V, I, I, I, I, V, V, V]),
    "isegmi_op_deform_im2col": (I, [V, I, I, I, I, V, I, I, I, I, I, V, V]),
    "isegmi_op_deform_im2col_v1": (I, [V, I, I, I, I, V, I, I, I, I, I, V, V]),
    "isegmi_op_deform_conv2d": (I, [V, I, I, I, I, V, I, I, I, V, I, V, V, V, I, V, V]),
    "isegmi_op_upsample_nearest2x_add": (I, [V, I, I, I, I, V, I, I, V, V]),
    "isegmi_op_group_norm_workspace_bytes": (L, [L, I, I, I, I]),
    "isegmi_op_group_norm": (I, [V, L, I, I, I, I, V, V, F, V, I, V, V, L, V]),
    "isegmi_op_pad_c3_to_c4": (I, [V, L, V, V]),
    "isegmi_op_map_f32": (I, [V, V, L, I, V]),
    "isegmi_op_maxpool_f16": (I, [V, I, I, I, I, I, I, I, I, V, V]),
    "isegmi_op_resize_bilinear_f16": (I, [V, I, I, I, I, I, I, V, I, V, V]),
    "isegmi_op_upsample_nearest2x_add_f16": (I, [V, I, I, I, I, V, I, I, V, V]),
    "isegmi_op_topk": (I, [V, L, I, I, I, V, I, V, V, V, V]),
    "isegmi_op_yolact_detect": (I, [V, V]),
    "isegmi_op_yolact_coeff_rows": (I, [I, V, V, V, I, I, I, I, I, V, V, V, I, I, V, V, I, V, V]),
    "isegmi_op_yolact_masks": (I, [V, V, V, V, I, I, I, I, I, I, I, V, V, V, V]),
    "isegmi_op_yolact_masks_win": (I, [V, V, V, V, I, I, I, I, I, I, I, V, V, V, V, V, I, I, V]),
    "isegmi_op_maskiou_conv1": (I, [V, I, I, I, V, V, V, V]),
    "isegmi_op_maskiou_rescore": (I, [V, I, I, I, I, V, V, V, V, V]),
    "isegmi_op_nms": (I, [V, V, I, I, F, I, I, I, V, V, V]),
    "isegmi_op_roi_align": (I, [V, V, V, V, I, V, V, I, I, I, I, I, I, I, I, I, V, V, V]),
    "isegmi_op_avgpool_full": (I, [V, L, I, I, V, V]),
    "isegmi_op_roi_align_f16": (I, [V, V, V, V, I, V, V, I, I, I, I, I, I, I, I, V, V]),
    "isegmi_op_roi_table_bytes": (L, [I, I, I, I]),
    "isegmi_op_roi_prep": (I, [V, V, I, I, V, V, V, I, I, I, I, I, I, I, V, V, V]),
    "isegmi_op_roi_align_ordered": (I, [V, V, V, V, I, V, V, V, V, I, I, I, I, I, I, V, V]),
    "isegmi_op_roi_align_f16_ordered": (I, [V, V, V, V, I, V, V, V, V, I, I, I, I, I, I, V, V]),
    "isegmi_op_box_postprocess": (I, [V, V]),
    "isegmi_op_mask_logits_select": (I, [V, I, I, I, V, V, V, V, V]),
    "isegmi_op_mask_logits_select_f16": (I, [V, I, I, I, V, V, V, V, V]),
    "isegmi_op_paste_masks": (I, [V, V, V, I, I, I, I, I, F, V, V]),
    "isegmi_op_paste_masks_win": (I, [V, V, V, I, I, I, I, I, F, V, V, I, V]),
    "isegmi_op_grid_anchors": (I, [V, I, I, I, I, V, V]),
    "isegmi_op_rpn_level": (I, [V, V, V, I, I, I, I, I, F, F, I, V, V, V, V, V, V, V, V, V]),
    "isegmi_op_rpn_levels_workspace": (I, [I, I, V, I, I, V, V]),
    "isegmi_op_rpn_levels": (I, [I, V, V, V, V, I, I, I, I, F, F, I, V, V, V, V, V, V, V, V, V, V, V]),
    "isegmi_op_retina_select_workspace": (L, [I, I, V, I, I, I]),
    "isegmi_op_retina_select": (I, [V, V]),
    "isegmi_op_retina_postprocess_workspace": (L, [I, I, I]),
    "isegmi_op_retina_postprocess": (I, [V, V]),
    "isegmi_op_bbox_aug_workspace": (L, [I, I]),
    "isegmi_op_bbox_aug_candidates": (I, [I, I, I, I, I, I, F, V, L, V, L, V, V, V, V, V, L, V, V, V, V, V, V]),
    "isegmi_op_yolo_slice_records": (I, [I]),
    "isegmi_op_yolo_select_workspace": (L, [I, I, V, I, I, I]),
    "isegmi_op_yolo_select": (I, [I, I, V, V, V, V, I, I, I, F, I, F, I, I, V, L, V, V, V, V, V, V]),
    "isegmi_op_concat_up2x": (I, [V, I, I, I, I, V, I, V, V]),
    "isegmi_op_maxpool_darknet": (I, [V, I, I, I, I, I, I, I, V, V]),
    "isegmi_op_spp_concat": (I, [V, I, I, I, I, I, V, V]),
    "isegmi_op_attention": (I, [V, I, I, I, V, V]),
    "isegmi_op_layer_norm": (I, [V, L, I, L, V, V, F, V, L, V]),
    "isegmi_op_gelu": (I, [V, V, L, I, V]),
    "isegmi_op_patchify": (I, [V, I, I, I, I, V, V]),
    "isegmi_op_class_softmax": (I, [V, I, I, V, V]),
    "isegmi_op_paint": (I, [V, I, I, V, I, I, I, V, I, V, I, V, V]),
    "isegmi_rle_workspace": (I, [I, I, I, I, I, V, V, V, V, V, V]),
    "isegmi_op_rle_encode": (I, [V, V]),
    "isegmi_op_pose2seg_letterbox": (I, [V, V, I, I, V, V, I, I, V, V]),
    "isegmi_op_pose2seg_fit": (I, [V, V, I, V, V, I, I, V, V, V, V, V, V]),
    "isegmi_op_pose2seg_align": (I, [V, I, I, I, V, V, I, V, I, V]),
    "isegmi_op_pose2seg_skeleton": (I, [V, I, V, I, I, V]),
    "isegmi_op_pose2seg_masks": (I, [V, V, V, V, V, I, I, I, I, V, V, V, V, V, V, V]),
    "isegmi_op_pose_handoff": (I, [V, V, V, V, V, I, I, I, F, F, I, V, V, V, V, V]),
    "isegmi_op_pose_scores": (I, [V, V, I, I, V, V]),
    "isegmi_engine_create": (I, [I, I, I, I, V]),
    "isegmi_engine_destroy": (I, [V]),
    "isegmi_engine_set_param": (I, [V, S, F]),
    "isegmi_engine_get_param": (I, [V, S, F, V, V]),
    "isegmi_engine_graph_stats": (I, [V, V, V, V]),
    "isegmi_engine_set_conv": (I, [V, S, I, I, I, I, V, V, V]),
    "isegmi_engine_set_conv_grouped": (I, [V, S, I, I, V, V, V]),
    "isegmi_engine_set_tensor": (I, [V, S, V, L]),
    "isegmi_yolact_forward": (I, [V, V, I]),
    "isegmi_maskrcnn_forward": (I, [V, V, V, I]),
    "isegmi_maskrcnn_forward_canvas": (I, [V, V, V, I, I, I]),
    "isegmi_maskrcnn_aug_begin": (I, [V, I, I]),
    "isegmi_maskrcnn_aug_view": (I, [V, V, V, I, I, I, I, V]),
    "isegmi_maskrcnn_aug_merge": (I, [V]),
    "isegmi_retinanet_forward": (I, [V, V, V, I]),
    "isegmi_retinanet_forward_canvas": (I, [V, V, V, I, I, I]),
    "isegmi_yolov3_forward": (I, [V, V, I]),
    "isegmi_vit_forward": (I, [V, V, I]),
    "isegmi_maskrcnn_paste": (I, [V, V, I, I]),
    "isegmi_pose2seg_forward": (I, [V, V, V, V, V, I]),
    "isegmi_pose2seg_body": (I, [V, V, V, I]),
    "isegmi_pose2seg_persons": (I, [V, V, V, V, V]),
    "isegmi_pose2seg_wait_persons": (I, [V, V]),
    "isegmi_engine_pose_handoff": (I, [V, V, F, F, I, V, V, V, V]),
    "isegmi_yolact_postprocess": (I, [V, I, I]),
    "isegmi_yolact_postprocess_sizes": (I, [V, V, I]),
    "isegmi_engine_sync": (I, [V]),
    "isegmi_engine_stream": (I, [V, V]),
    "isegmi_engine_upload_async": (I, [V, V, V, L]),
    "isegmi_engine_preprocess_u8": (I, [V, V, I, I, I, V, I, I, I, I, L, V, V, I]),
    "isegmi_engine_preprocess_u8_flip": (I, [V, V, I, I, I, V, I, I, I, I, L, V, V, I, I]),
    "isegmi_engine_resample_u8": (I, [V, V, L, L, V, I, L, L, L, V, I, I, I, L, V, V, I, F]),
    "isegmi_engine_mark_step": (I, [V]),
    "isegmi_engine_step_times": (I, [V, V, I, V]),
    "isegmi_engine_wait_mark": (I, [V, I]),
    "isegmi_engine_buffer_info": (I, [V, S, V, V, V, V, V]),
    "isegmi_engine_memory": (I, [V, V, V]),
    "isegmi_engine_stream_layout": (I, [V, V, I]),
    "isegmi_engine_lane_layout": (I, [V, V, I]),
    "isegmi_engine_get_timings": (I, [V, V, I, V, I, V]),
    "isegmi_engine_rle": (I, [V, V]),
    "isegmi_engine_coco_record_bytes": (I, [V, I, V, V]),
    "isegmi_engine_pack_coco_records": (I, [V, V, L, I, V]),
    "isegmi_engine_pack_box_records": (I, [V, V, V, L, I, V]),
    "isegmi_engine_pack_keypoint_records": (I, [V, V, V, L, I, V]),
    "isegmi_engine_paint": (I, [V, I, V, I, I, V, I, V, I, V]),
    "isegmi_engine_download_async": (I, [V, I, V, V, L]),
    "isegmi_engine_download_fence": (I, [V, I]),
    "isegmi_engine_download_wait": (I, [V, I]),
    "isegmi_yolact_pack_records": (I, [V, V, L, I, V]),
    "isegmi_maskrcnn_pack_records": (I, [V, V, L, V]),
    "isegmi_engine_conv_stats": (I, [V, V, V, V]),
    "isegmi_engine_op_stats": (I, [V, V, I, V, V, V, I, V]),
    "isegmi_engine_conv_report": (I, [V, V, I]),
    "isegmi_coco_rle_prefix_bytes": (I, [L, I, V, V, V, V]),
    "isegmi_op_rle_prefix": (I, [V, V, V, I, V, V, V, V, V]),
    "isegmi_op_rle_iou": (I, [V, V, V, V, V, V, I, V, L, V, V]),
    "isegmi_op_bbox_iou": (I, [V, I, V, L, V, V]),
    "isegmi_op_oks": (I, [V, V, V, V, I, I, V, L, V, V]),
    "isegmi_coco_match_bytes": (I, [L, L, I, I, V, V, V, V]),
    "isegmi_op_coco_match": (I, [V, V]),
    "isegmi_comm_unique_id": (I, [V]),
    "isegmi_comm_create": (I, [V, I, I, V]),
    "isegmi_comm_destroy": (I, [V]),
    "isegmi_comm_allgather": (I, [V, V, V, L, V]),
    "isegmi_comm_wait": (I, [V]),
    "isegmi_comm_fence_producer": (I, [V, I, V]),
    "isegmi_comm_allgather_slot": (I, [V, I, V, V, L, V]),
    "isegmi_comm_wait_slot": (I, [V, I]),
    "isegmi_comm_info": (I, [V, V]),
}


def declare(lib):
    """Set restype / argtypes of every function of the table on a loaded CDLL.  -> the names the library does not export."""
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        f.restype, f.argtypes = res, args
    return missing
