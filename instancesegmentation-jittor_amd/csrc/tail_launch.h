// tail_launch.h -- host-side launchers of the detection tail that other translation units call: csrc/select.hip (top-k), csrc/rcnn_ops.hip (RPN, RoIAlign,
// box / mask heads' tails) and csrc/retinanet_ops.hip.  The ONLY declaration of each; default arguments are stated here.  engine.h includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isegmi.h"

namespace isegmi {

// ---- csrc/select.hip
int topk_launch(const float* keys, int64_t row_stride, int rows, int n, int k, const int* limit, int rows_per_limit,
                float* out_vals, int* out_idx, int* out_cnt, hipStream_t st);
int64_t topk_scratch_elems(int rows, int n, int k);
int topk_launch_ws(const float* keys, int64_t row_stride, int rows, int n, int k, const int* limit, int rows_per_limit, float* out_vals,
                   int* out_idx, int* out_cnt, float* ws_vals, int* ws_idx, hipStream_t st);
int topk_segmented_launch(const float* keys, int64_t row_stride, int rows, int nseg, int seg_len, int seg_take, int k, const int* limit,
                          int rows_per_limit, float* out_vals, int* out_idx, int* out_cnt, hipStream_t st);
// RPN selection batched over (level, image) (round 5): the grouped two-level top-k here, the five launches for all levels in csrc/rcnn_ops.hip
constexpr int RPN_MAX_LEVELS = 5;
int rpn_topk_plan(int nl, int N, const int* n, int k, int* slices, int64_t* cand_off);
int rpn_topk_levels_launch(int nl, int N, const float* keys, const int64_t* key_off, const int* n, int k, const int* slices, const int64_t* cand_off,
                           float* cand_vals, int* cand_idx, float* out_vals, int* out_idx, int* out_cnt, hipStream_t st);

// ---- csrc/rcnn_ops.hip
int rpn_levels_workspace(int nl, int N, const int* HWA, int pre_nms, int64_t* prob_elems, int64_t* cand_elems);
int rpn_levels_select_launch(int nl, const float* const* heads, const float* const* anchors, const int* HWA, const int* level_slot, const int* image_hw, int N,
                             int A, int CH, int pre_nms, int post_nms, float thr, float min_size, int ge, int L, int post_cap, float* prob, float* cand_vals,
                             int* cand_idx, float* tk_vals, int* tk_idx, int* tk_cnt, void* nms_ws, float* out_boxes, float* out_scores, int* out_cnt,
                             hipStream_t st);
int nms_launch(const float* boxes, const float* scores, int problems, int n, float thr, int plus_one, int ge, int max_keep, int* keep,
               int* cnt, hipStream_t st);
int grid_anchors_launch(const float* base, int A, int stride, int gh, int gw, float* out, hipStream_t st);
int rpn_sigmoid_launch(const float* head, int64_t total, int A, int CH, float* prob, hipStream_t st);
int rpn_decode_nms_launch(const float* head, const float* anchors, const float* tk_vals, const int* tk_idx, const int* tk_cnt,
                          const int* image_hw, int N, int HWA, int A, int CH, int pre_nms, int post_nms, float thr, float min_size,
                          int ge, int level, int L, int post_cap, float* out_boxes, float* out_scores, int* out_cnt, void* nms_ws,
                          hipStream_t st);
int sum_counts_launch(const int* cnt, int N, int L, int* total, hipStream_t st);
int gather_proposals_launch(const float* cand_boxes, const float* fin_vals, const int* fin_idx, const int* fin_cnt, int N,
                            int cand_per_img, int K, float* props, float* prop_scores, int* prop_cnt, hipStream_t st);
int roi_align_launch(const float* const* feats, const int* Hs, const int* Ws, const float* scales, int nlevels, const float* rois,
                     const int* counts, int N, int K, int C, int PH, int PW, int g, int k_min, int fixed_level, float* out,
                     int* out_level, hipStream_t st, const int* order = nullptr, const void* tab = nullptr, int aligned = 0);
int roi_prep_launch(const float* rois, const int* counts, int N, int K, const int* Hs, const int* Ws, const float* scales, int nlevels, int k_min, int C,
                    int PH, int PW, int esize, int* order, void* tab, hipStream_t st, int aligned = 0);
int avgpool_full_launch(const float* x, int64_t R, int HW, int C, float* out, hipStream_t st);
int box_postprocess_launch(const isegmi_box_post_args* a, hipStream_t st);
int mask_logits_select_launch(const float* feat, int R, int HW, int C, const float* w, const float* b, const int* labels, float* out,
                              hipStream_t st);
int paste_masks_launch(const float* masks, const float* boxes, const int* counts, int N, int K, int M, int im_h, int im_w, float thr,
                       uint8_t* out, hipStream_t st, int* win, bool clear);
int scale_boxes_launch(const float* boxes, const float* ratios, int N, int K, float* out, hipStream_t st);

// ---- csrc/retinanet_ops.hip
int64_t retina_select_workspace_bytes(int nl, int N, const int* HW, int A, int C, int top_n);
int retina_select_launch(const isegmi_retina_select_args* p, hipStream_t st);
int64_t retina_post_workspace_bytes(int N, int nseg, int seg_len);
int retina_postprocess_launch(const isegmi_retina_post_args* p, hipStream_t st);

// ---- csrc/bbox_aug.hip
int64_t bbox_aug_workspace_bytes(int N, int R);
struct BBoxAugArgs {   // isegmi_op_bbox_aug_candidates' arguments (include/isegmi.h says what each one is)
    int N, R, ncls, cls_agnostic, hflip, cap;
    float score_thresh;
    int64_t logits_stride, regr_stride, ws_bytes;
    const float *d_logits, *d_regr, *d_props, *d_ratios_wh;
    const int *d_prop_cnt, *d_image_hw;
    void* d_ws;
    float *d_pool_boxes, *d_pool_scores;
    int *d_pool_labels, *d_pool_cnt, *d_pool_total;
};
int bbox_aug_candidates_launch(const BBoxAugArgs* p, hipStream_t st);

// ---- csrc/yolo_ops.hip
int yolo_slice_records(int C);   // anchor records per slice of yolo_select's first launch (-1: C outside 1..256)
int64_t yolo_select_workspace_bytes(int nl, int N, const int* grid_hw, int A, int C, int top_n);
int yolo_select_launch(int nl, int N, const float* const* d_heads, const int* grid_hw, const int* strides, const float* anchors_wh, int A, int C, int top_n,
                       float conf_thresh, int multi_label, float min_wh, int canvas_w, int canvas_h, void* d_ws, int64_t ws_bytes, float* d_out_boxes,
                       float* d_out_scores, int* d_out_labels, int* d_out_cnt, int* d_out_total, hipStream_t st);
int concat_up2x_launch(const float* coarse, int N, int Hc, int Wc, int Cc, const float* skip, int Cs, float* out, hipStream_t st);

// ---- csrc/yolo_pool.hip
int maxpool_darknet_launch(const float* in, int N, int H, int W, int C, int size, int stride, int zero_pad, float* out, hipStream_t st);
int spp_concat_launch(const float* in, int N, int H, int W, int C, int zero_pad, float* out, hipStream_t st);

// ---- csrc/keypoint_ops.hip
int keypoint_heatmap_launch(const float* in, int64_t R, int Hi, int Wi, int K, float* out, hipStream_t st);
int keypoint_decode_launch(const float* heat, const float* boxes, const int* count, int N, int cap, int S, int K, float* kpt, float* kscore, hipStream_t st);

}  // namespace isegmi
