// engine.h -- model engine: packed-weight registry, named activation buffers, per-model forward graphs (yolact.cpp, maskrcnn.cpp, pose2seg.cpp, retinanet.cpp, yolov3.cpp, vit.cpp).
#pragma once
#include "tail_launch.h"
#include <stdarg.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/isegmi.h"
#include "common.h"

#define TRY(x)               \
    do {                     \
        int _rc = (x);       \
        if (_rc) return _rc; \
    } while (0)

namespace isegmi {

struct Tensor {
    float* d = nullptr;
    int N = 0, H = 0, W = 0, C = 0;
    int dt = 0;  // 0 fp32, 1 fp16 storage
    int64_t numel() const { return (int64_t)N * H * W * C; }
};

struct ConvLayer {
    int Cout = 0, R = 0, S = 0, Cin = 0;
    float* d_w = nullptr;      // packed (fp32 image, or fp16 image when f16)
    bool f16 = false;
    float* d_scale = nullptr;  // may be null (=1)
    float* d_shift = nullptr;  // may be null (=0)
    int groups = 1;            // > 1: a grouped 3x3 (ResNeXt conv2): d_w is the isegmi_pack_conv_weights_grouped image of [Cout][3][3][Cin / groups] weights
    bool view = false;         // a row range of another layer: d_w / d_scale / d_shift point into ITS allocations (never freed, never counted)
};

struct RawBuf {
    void* d = nullptr;
    int64_t bytes = 0;
    std::vector<int64_t> shape;
    int dtype = 0;  // 0 f32, 1 i32, 2 u8, 3 i64
};

struct StageTime {
    std::string name;
    hipEvent_t ev;
};

// default of the "step_overlap" engine parameter (Yolact fp32 only; profiles/step_overlap.md has the measurement behind it)
constexpr float STEP_OVERLAP_DEFAULT = 1.0f;

struct Engine {
    int kind = 0;  // 1 yolact, 2 maskrcnn, 3 pose2seg, 4 retinanet, 5 yolov3, 7 vit (6 is refused)
    int max_batch = 0, H = 0, W = 0;       // H, W: the LARGEST network input (padded canvas) this engine serves
    int cur_H = 0, cur_W = 0;              // Mask R-CNN: padded canvas of the current forward (<= H, W; to_image_list pads each batch to its own size)
    int anchor_H = -1, anchor_W = -1;      // canvas the anchors.* buffers were generated for
    hipStream_t stream = nullptr;          // main stream (all results are complete on it when a forward returns)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};  // side streams for independent branches
    hipStream_t cur = nullptr;             // stream the next launch goes to
    hipStream_t tail = nullptr;            // Yolact Detect + postprocess: latency-bound tail, overlapped with the NEXT forward's backbone
    hipEvent_t tail_done = nullptr;        // recorded after the last tail launch; the next forward's head/proto writers wait on it
    bool tail_pending = false;
    // Yolact cross-step pipelining: FPN + protonet + prediction heads of step i run on their own stream group while step i+1's
    // backbone already runs on the main stream (the backbone chain of mid-size layers leaves CUs idle that the heads' large
    // layers fill).  lat_done fences the only backbone buffers the heads phase reads (C3-C5, by the lateral convs).
    hipStream_t heads = nullptr;
    hipStream_t hside[3] = {nullptr, nullptr, nullptr};
    hipEvent_t lat_done[2] = {nullptr, nullptr};   // one per backbone lane (see below): the laterals that read THAT lane's C3-C5
    bool lat_pending[2] = {false, false};
    hipEvent_t heads_done = nullptr;       // end of the last pipelined heads phase (a non-pipelined forward's heads phase waits on it)
    bool heads_pending = false;
    bool multi_stream = true;
    // Yolact fp32 "step_overlap": two backbone LANES.  A lane is a main stream with its three side streams plus its own copy of every buffer a
    // forward writes before the tail WAR point (padded input, stem, pooled map, the res<l>.* activations, laterals, P3-P7; lane 1's carry the
    // suffix "@1").  Consecutive forwards alternate lanes, so step i + 1's backbone overlaps step i's backbone, heads and tail; everything
    // behind the WAR point (heads, protonet, Detect, postprocess) has one set of buffers and keeps running in step order.  `stream` / `side`
    // are the CURRENT lane's streams while a forward is enqueued and lane 0's otherwise.
    hipStream_t lane_stream[2] = {nullptr, nullptr};
    hipStream_t lane_side[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int lane_state = 0;                    // 0: lane 1's streams not asked for yet; 1: dealt; -1: the runtime gave no free queue -- one lane (reported)
    int lane = 0;                          // lane of the forward being enqueued
    int lane_next = 0;                     // engine-side counter: forwards alternate lanes while step_overlap is active
    int last_lanes = 1;                    // lanes the last forward could choose from (1: step_overlap inactive)
    bool lane1_busy = false;               // lane 1 has run a forward since the last sync
    int64_t lane1_forwards = 0;
    std::string lane_tag;                  // appended to the names eng_act allocates: "" or "@1" before the WAR point, "" behind it
    // hipGraph replay of a forward ("graph" param): the ~130-150 launches of one forward are captured once per
    // (entry, batch, input pointer) and replayed with one hipGraphLaunch -- removes the per-launch gaps that bound bs=1
    // latency.  A replay ends joined on the main stream (no cross-step tail overlap), so it is a latency mode.
    bool capturing = false;
    std::map<std::string, hipGraphExec_t> graphs;
    std::map<std::string, int> graph_warm;
    int64_t graph_captures = 0, graph_replays = 0, graph_failures = 0;
    // asynchronous input upload (isegmi_engine_upload_async): pinned host -> device on a copy stream; in_done marks the point
    // where the last forward has consumed its input buffer (WAR for the next upload; recorded at the end of a hipGraph replay)
    hipStream_t copy = nullptr;
    hipEvent_t in_done[2] = {nullptr, nullptr};   // per lane: the two lanes' forwards are not ordered against each other
    bool in_pending[2] = {false, false};
    // one completion event per upload destination (input slot / uint8 staging buffer): the consumer of a buffer waits for ITS upload
    // only, so the copy of batch i+1 really overlaps forward i
    // (waited: bit l = lane l's main stream has been ordered behind it; two lanes may read one input slot, each needs its own wait)
    struct Upload { const char* dst = nullptr; int64_t bytes = 0; hipEvent_t done = nullptr; unsigned waited = ~0u; };
    unsigned lane_mask() const { return lane_state == 1 ? 3u : 1u; }
    bool consumed(const Upload& u) const { return (u.waited & lane_mask()) == lane_mask(); }
    std::vector<Upload> uploads;
    // per-step completion marks on the results stream (isegmi_engine_mark_step / _step_times): true per-step latency samples
    std::vector<hipEvent_t> step_marks;
    // small host arrays that change from step to step (image sizes, resize ratios) reach the device through a ring of pinned slots: a
    // truly asynchronous copy on the consumer's own stream instead of a synchronous hipMemcpy of pageable memory
    char* pin_ring = nullptr;
    static constexpr int PIN_SLOTS = 32, PIN_SLOT_BYTES = 4096;
    hipEvent_t pin_ev[PIN_SLOTS] = {};
    bool pin_used[PIN_SLOTS] = {};
    int pin_next = 0;
    int hw_slot = 0;                       // Mask R-CNN image_hw lives in two device buffers used alternately (WAR against the previous forward's tail)
    // asynchronous download of a step's record block (device-side COCO output) on its own stream: two slots, like the RCCL records
    void* stream_set = nullptr;  // the pooled set the ten streams below belong to (engine.cpp: acquire_streams / release_streams)
    hipEvent_t dl_done[2] = {nullptr, nullptr};
    bool dl_used[2] = {false, false};
    bool fp16 = false;                     // fp16 storage + f16 MFMA convs (BASELINE configs[4]); set before loading weights
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    std::map<std::string, ConvLayer> convs;
    std::map<std::string, RawBuf> tensors;   // user-set constant tensors (priors, anchors, deconv weights ...)
    std::map<std::string, RawBuf> bufs;      // activations / workspaces / outputs, allocated on first use
    std::map<std::string, float> params;
    bool finalized = false;
    std::vector<int32_t> last_hw;      // host copies of the small per-batch inputs already resident on the device
    const void* last_hw_ptr = nullptr;
    std::vector<float> last_ratios;
    const void* last_ratios_ptr = nullptr;
    int last_N = 0;
    // test-time box augmentation: batch and pool slots of the sequence isegmi_maskrcnn_aug_begin opened (0: none open), the views it has
    // taken, and view 0's image sizes, which aug_merge makes current again
    int aug_N = 0, aug_cap = 0, aug_views = 0;
    std::vector<int32_t> aug_hw0;
    // Pose2Seg in two halves: what isegmi_pose2seg_body leaves for isegmi_pose2seg_persons -- the batch's image sizes and P2 -- and, per
    // device keypoint buffer a producer stream fills, the event behind the last persons call that read it (isegmi_pose2seg_wait_persons)
    std::vector<int32_t> p2s_hw;
    Tensor p2s_p2;
    std::map<const void*, hipEvent_t> p2s_kpts_read;
    // Yolact fp32 "lazy_coeffs": the forward runs only the loc|conf rows of the fused head and computes the mask coefficients of the kept detections on
    // the tail stream; columns [85 A, 117 A) of `headcat` then hold nothing until a fetch of that buffer asks for them (yolact_fill_coeff_columns).
    bool coeff_cols_valid = true;
    // ViT (vit.cpp): the vit.tokens allocation whose class rows (row 0 of every image = vit.cls_row) are written; set_tensor clears it
    const void* vit_cls_rows_in = nullptr;
    // timing
    bool timing = false;
    std::vector<StageTime> marks;
    std::vector<std::pair<std::string, float>> last_times;
    // per-conv-launch HIP-event timing (roofline measurement): accumulated until read
    bool conv_timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> conv_evs;
    std::vector<std::pair<std::string, double>> conv_ev_info;  // (label, flops) per pending event pair
    bool conv_trace = false;  // param "conv_trace": one stderr line per conv launch
    std::map<std::string, std::pair<double, double>> conv_layers;  // label -> (flops, ms) accumulated
    double conv_flops_pending = 0, conv_flops = 0, conv_ms = 0;
    int64_t conv_launches = 0;
    // HIP-event timing of the HBM-bound (non-conv) stages with their ALGORITHMIC bytes (SURVEY 8d "Algorithmic bytes"): param "op_timing";
    // isegmi_engine_op_stats accumulates and returns (label, us, bytes, launches) -- bench.py's roofline_hbm
    bool op_timing = false;
    struct OpEv { hipEvent_t a, b; const char* label; double bytes; };
    std::vector<OpEv> op_evs;
    struct OpStat { double us = 0, bytes = 0; int64_t launches = 0; };
    std::map<std::string, OpStat> op_stats;

    float param(const std::string& k, float def) const {
        auto it = params.find(k);
        return it == params.end() ? def : it->second;
    }
};

// engine.cpp helpers
int eng_buf(Engine& e, const std::string& name, int64_t bytes, void** out, int dtype = 0,
            std::vector<int64_t> shape = {});
int eng_act(Engine& e, const std::string& name, int N, int H, int W, int C, Tensor* t, int dt = 0);
int eng_conv(Engine& e, const std::string& layer, const Tensor& in, int stride, int pad, int act, const Tensor* residual,
             const std::string& out_name, Tensor* out, bool out_f32 = false, bool may_split = false);
// runs `body` (a forward's enqueue code) eagerly or, with the "graph" parameter, as a captured hipGraph keyed by `key`
int eng_graph_run(Engine& e, const std::string& key, const std::function<int()>& body);
void eng_graph_reset(Engine& e);
int eng_tail_end(Engine& e);
int eng_input_consumed(Engine& e);  // call right after the last kernel that reads the caller's input buffer
int eng_wait_upload(Engine& e, const void* d_ptr, int64_t bytes, hipStream_t st);  // st waits for every pending upload / front-end write into [d_ptr, d_ptr + bytes)
int eng_stage_small(Engine& e, const void* h_src, size_t bytes, void* d_dst, hipStream_t st);  // host array -> pinned ring slot -> async H2D on st
hipStream_t eng_results_stream(Engine& e);  // the stream the last forward's results complete on
int eng_bottleneck_f16(Engine& e, const std::string& block, const Tensor& x, bool first, const std::string& out_name, Tensor* out, bool* fused);
int eng_conv_up2x_f16(Engine& e, const std::string& layer, const Tensor& x, const Tensor& coarse, const std::string& out_name, Tensor* out, bool* merged);
// several independent convolutions of one point of the graph as ONE launch (fp32: conv2d_group_launch; fp16, a forced tile, a single member or
// "conv_groups" 0: one launch per member, as eng_conv / eng_conv_into would issue them)
struct ConvGroupItem {
    std::string layer;
    Tensor in;
    int stride = 1, pad = 0, act = 0;
    const Tensor* residual = nullptr;
    std::string out_name;            // named activation (eng_conv) ...
    Tensor* out = nullptr;
    void* dst = nullptr;             // ... or an explicit strided destination (eng_conv_into)
    int out_div = 0;
    int64_t out_img_stride = 0, out_pix_stride = 0;
    bool out_f32 = false;
};
int eng_conv_group(Engine& e, std::vector<ConvGroupItem>& items);
int conv2d_group_launch(int n, const isegmi_conv_desc* const* d, const float* const* in, const float* const* w, const float* const* scale,
                        const float* const* shift, const float* const* res, float* const* out, hipStream_t st);
int eng_rpn_head_f16(Engine& e, const std::string& conv, const std::string& headl, const Tensor& x, const std::string& out_name, Tensor* out, bool* fused);
int eng_stem_pool_f16(Engine& e, const std::string& layer, const Tensor& halo, int H, int W, const std::string& out_name, Tensor* out, bool* fused);
int eng_conv_stem_f16(Engine& e, const std::string& layer, const Tensor& halo, int H, int W, const std::string& out_name, Tensor* out);
// conv writing into a caller-provided strided destination (heads -> concatenated buffers, deconv parities)
// (residual: contiguous [M][Cout], whatever the destination's strides)
int eng_conv_into(Engine& e, const std::string& layer, const Tensor& in, int stride, int pad, int act, void* dst, int out_div,
                  int64_t out_img_stride, int64_t out_pix_stride, bool out_f32 = false, const float* residual = nullptr);
void eng_mark(Engine& e, const char* name);
// fork(k): side stream k waits for everything queued on the main stream so far; join(k): main waits for side k.
int eng_fork(Engine& e, int k);
int eng_join(Engine& e, int k);
// RAII: launches inside the scope go to side stream k (no-op when multi_stream is off)
struct SideScope {
    Engine& e;
    hipStream_t saved;
    SideScope(Engine& e_, int k) : e(e_), saved(e_.cur) { if (e.multi_stream) e.cur = e.side[k]; }
    ~SideScope() { e.cur = saved; }
};

// RAII: brackets the launches of one HBM-bound stage with HIP events on the stream they go to (no-op unless "op_timing" is set)
struct OpScope {
    Engine& e;
    hipStream_t st;
    const char* label;
    double bytes;
    hipEvent_t a = nullptr;
    OpScope(Engine& e_, hipStream_t st_, const char* label_, double bytes_) : e(e_), st(st_), label(label_), bytes(bytes_) {
        if (e.op_timing && !e.capturing && hipEventCreate(&a) == hipSuccess) (void)hipEventRecord(a, st);
    }
    ~OpScope() {
        if (!a) return;
        hipEvent_t b = nullptr;
        if (hipEventCreate(&b) == hipSuccess) { (void)hipEventRecord(b, st); e.op_evs.push_back({a, b, label, bytes}); }
        else (void)hipEventDestroy(a);
    }
};

// RAII: one conv-type launch (or one grouped launch) on e.cur.  With "conv_timing" it brackets the launch with a HIP event pair, which done() hands
// to conv_report / conv_stats with the launch's label and algorithmic FLOPs; with "conv_trace", trace() prints the launch's `convlaunch` line (one
// per member of a grouped launch).  A scope left without done() -- an error, or nothing launched -- destroys its events: no half-recorded pair.
struct ConvScope {
    Engine& e;
    hipEvent_t a = nullptr, b = nullptr;
    explicit ConvScope(Engine& e_) : e(e_) {
        if (!e.conv_timing) return;
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, e.cur) == hipSuccess) return;
        drop();
    }
    ~ConvScope() { drop(); }
    void drop() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
    }
    // dev tools (tools/conv_traffic.py): the launch order, to join per-dispatch counters with layers
    void trace(const std::string& layer, const char* suffix, int N, int H, int W, int Cin, int Cout, int R, int stride, int M, bool res) const {
        if (e.conv_trace) fprintf(stderr, "convlaunch\t%s%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", layer.c_str(), suffix, N, H, W, Cin, Cout, R, stride, M, res ? 1 : 0);
    }
    __attribute__((format(printf, 3, 4))) void done(double flops, const char* label_fmt, ...) {
        if (!a) return;
        char label[320];
        va_list ap;
        va_start(ap, label_fmt);
        vsnprintf(label, sizeof(label), label_fmt, ap);
        va_end(ap);
        (void)hipEventRecord(b, e.cur);
        e.conv_evs.push_back({a, b});
        e.conv_ev_info.push_back({label, flops});
        e.conv_flops_pending += flops;
        a = b = nullptr;
    }
};

// resnet.cpp: the ResNet trunk every model's backbone (and the C4 RoI head) is built from
// Stem: d_images [N][H][W][3] fp32 -> padded 4-channel copy ("input4"; fp16: the zero-haloed "input4h") -> 7x7/2 conv `layer` + BN + ReLU ("stem") ->
// 3x3/2 max-pool ("pool").  fp16: conv and pool as one launch where eng_stem_pool_f16 has the kernel ("stem" then never exists).
int resnet_stem(Engine& e, const std::string& layer, const float* d_images, int N, int H, int W, Tensor* pool);
// One stage of bottleneck blocks: block b's layers are <layers>.<b>.{conv1, conv2, conv3, downsample.0}.
struct ResStage {
    std::string layers;          // layer-name prefix
    std::string bufs;            // buffer-name prefix of the per-block buffers <bufs>.<b>.{t1, t2, ds, out}: `layers`, unless one set of weights runs into two sets of buffers
    int blocks = 0;
    int stride = 1;              // of block 0
    bool stride_in_1x1 = false;  // the stride sits on conv1 (maskrcnn-benchmark's STRIDE_IN_1X1) instead of on the 3x3 (torchvision, Yolact)
    // full: the FPN backbones' form -- buffers by liveness under `stage`.{t1, t2, outA, outB, C} (unless "alias_buffers" is 0), block 0's projection
    // grouped with conv1 (fp32) or on side stream 0, the fused fp16 bottleneck where it has a kernel, `conv_split_k` marks.  Otherwise the plain
    // form: one launch per layer on the current stream, one buffer per layer.
    bool full = false;
    std::string stage;           // full: "res<l>"
    bool proj_by_name = false;   // a block projects its shortcut where it has a downsample.0 (torchvision-form weights of any layout); otherwise block 0 does
    hipEvent_t before_out = nullptr;  // the main stream waits on it before the launch that writes the stage's final output
};
int resnet_stage(Engine& e, const ResStage& s, const Tensor& in, Tensor* out);
// GroupNorm layers.  The norm is data: a convolution `layer` whose GroupNorm affine was set as the tensors <layer>.gn.weight / .gn.bias
// (the host sets them where the state dict's norm has a weight but no running statistics) is followed by eng_gn as its own launch, in place on the
// convolution's output; the convolution itself then runs with scale 1, shift 0 and no activation.  Groups per layer: C / "gn_dim_per_gp" where that
// parameter is positive, else "gn_num_groups" (32); eps "gn_epsilon" (1e-5).  fp32 only.
bool eng_has_gn(Engine& e, const std::string& layer);
int eng_gn(Engine& e, const std::string& layer, Tensor* x, const Tensor* residual, bool relu);

// darknet.cpp: the Darknet-53 trunk of yolact_darknet53_config and YOLOv3 -> C[0..2] at strides 8, 16, 32; before_c3: waited on before C[0] is overwritten
int darknet_backbone(Engine& e, const std::string& prefix, const float* d_images, int N, Tensor* C, hipEvent_t before_c3);
// the seven-convolution trunk of yolov3-tiny -> *skip (256 channels, stride 16), *top (1024, stride 32); zero_pad: the pad switch of its max-pools
int darknet_tiny_backbone(Engine& e, const std::string& prefix, const float* d_images, int N, int zero_pad, Tensor* skip, Tensor* top);
int yolact_forward(Engine& e, const float* d_images, int N);
int yolact_postprocess(Engine& e, int h, int w, const int32_t* h_image_hw = nullptr);
// "lazy_coeffs" (yolact.cpp): the two row-range views of the fused head, whether a forward of N images takes the lazy schedule, and the fill of headcat's
// coefficient columns on demand
constexpr const char* kHeadCat = "prediction_layers.0.head_cat";
constexpr const char* kHeadCatLocConf = "prediction_layers.0.head_cat[loc|conf]";
constexpr const char* kHeadCatCoeff = "prediction_layers.0.head_cat[coeff]";
constexpr int kYolactClasses = 81, kYolactMaskDim = 32;
void yolact_head_views(Engine& e);
bool yolact_lazy_coeffs(Engine& e, int N);
int yolact_fill_coeff_columns(Engine& e);
int maskrcnn_forward(Engine& e, const float* d_images, int N);
// maskrcnn.cpp: what the R-CNN graphs, retinanet.cpp and the results stage share
int maskrcnn_set_image_hw(Engine& e, const int32_t* h_image_hw, int N);
int maskrcnn_det_cap(Engine& e);
int maskrcnn_nms_flags(Engine& e);
int rcnn_trunk(Engine& e, const float* d_images, int N, bool full, Tensor* C);
int level_anchors(Engine& e, int l, const RawBuf& base, int A, int gh, int gw, int64_t cap_cells, bool regen, const float** out);
int rcnn_canvas_check(Engine& e, int N, int H, int W);
int rcnn_begin_canvas(Engine& e, const float* d_images, const int32_t* h_image_hw, int N, int H, int W);
int pose2seg_det_cap(Engine& e);  // pose2seg.cpp
int eng_next_event(Engine& e, hipEvent_t* ev);
int maskrcnn_paste(Engine& e, const float* h_ratios_wh, int out_h, int out_w);
bool maskrcnn_mask_on(Engine& e);
bool maskrcnn_keypoint_on(Engine& e);
int maskrcnn_num_keypoints(Engine& e);
int maskrcnn_stage_ratios(Engine& e, const float* h_ratios_wh, int N, hipStream_t ps, void** d_ratios);

// kernels implemented in other translation units (the detection tail's launchers: tail_launch.h)
int conv2d_launch(const isegmi_conv_desc* d, const float* in, const float* w, const float* scale, const float* shift,
                  const float* res, float* out, hipStream_t st);
int conv2d_grouped_launch(const isegmi_conv_desc* d, int groups, const float* in, const float* w, const float* scale, const float* shift, const float* res,
                          float* out, hipStream_t st);
int conv2d_f16_launch(const isegmi_conv_desc* d, const void* in, const void* w, const float* scale, const float* shift, const void* res,
                      void* out, int out_f32, hipStream_t st);
int conv2d_f16_up2x_launch(const isegmi_conv_desc* d, const void* in, const void* w, const float* scale, const float* shift, const void* coarse, int Hc, int Wc,
                           void* out, hipStream_t st);
int conv2d_f16_head_launch(const isegmi_conv_desc* d, const void* in, const void* w, const float* scale, const float* shift, const void* w2,
                           const float* scale2, const float* shift2, int cout2, float* out2, bool* fused, hipStream_t st);
bool stem_pool_f16_supported(int Cout);
int stem_pool_f16_launch(int N, int H, int W, const void* halo, const void* w, const float* scale, const float* shift, void* out, int flags, hipStream_t st);
bool bottleneck_f16_supported(int Cin, int Cmid);
bool bottleneck_f16_ds_supported(int Cin, int Cmid);
int bottleneck_f16_launch(const isegmi_bottleneck_desc* d, const void* x, const void* w1, const float* s1, const float* b1, const void* w2,
                          const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, const void* wd, const float* sd,
                          const float* bd, void* out, hipStream_t st);
int pad_c3_to_f16_halo_launch(const float* in, int N, int H, int W, void* out, hipStream_t st);
int resize_bilinear_f16_launch(const void* in, int N, int H, int W, int C, int Ho, int Wo, const void* add, int relu, void* out, hipStream_t st);
int maxpool_to_f16_launch(const void* in, int in_f16, int N, int H, int W, int C, int k, int s, int p, void* out, hipStream_t st);
int nearest2x_add_f16_launch(const void* coarse, int N, int Hc, int Wc, int C, const void* lat, int H, int W, void* out, hipStream_t st);
int roi_align_f16_launch(const void* const* feats, const int* Hs, const int* Ws, const float* scales, int nlevels, const float* rois,
                         const int* counts, int N, int K, int C, int PH, int PW, int g, int k_min, void* out, hipStream_t st,
                         const int* order = nullptr, const void* tab = nullptr, int aligned = 0);
int mask_logits_select_f16_launch(const void* feat, int R, int HW, int C, const float* w, const float* b, const int* labels, float* out,
                                  hipStream_t st);
int maxpool_launch(const float* in, int N, int H, int W, int C, int k, int s, int p, float* out, hipStream_t st);
int64_t groupnorm_workspace_bytes(int64_t N, int H, int W, int C, int groups);
bool groupnorm_is_slab(int H, int W);
int groupnorm_launch(const float* x, int64_t N, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, const float* residual,
                     int relu, float* out, void* ws, int64_t ws_bytes, hipStream_t st);
int resize_bilinear_launch(const float* in, int N, int H, int W, int C, int Ho, int Wo, const float* add, int relu, float* out,
                           hipStream_t st);
int nearest2x_add_launch(const float* coarse, int N, int Hc, int Wc, int C, const float* lat, int H, int W, float* out,
                         hipStream_t st);
int maskiou_conv1_launch(const float* lo, int NK, int PH, int PW, const float* w, const float* b, float* out, hipStream_t st);
int maskiou_rescore_launch(const float* feat, int N, int K, int HW, int C, const int* cls, const float* score, const int* count,
                           float* out, hipStream_t st);
int deform_im2col_launch(const float* x, int N, int H, int W, int C, const float* om, int R, int S, int stride, int pad, int dil, int modulated,
                         float* out, hipStream_t st);
// fused 3x3 deformable convolution (csrc/deform_conv.hip): `w` is the isegmi_pack_conv_weights image of the 1x1 / 9*C descriptor
int deform_conv2d_launch(const float* x, int N, int H, int W, int C, const float* om, int OC, int modulated, int stride, const float* w, int Cout,
                         const float* scale, const float* shift, const float* res, int act, float* out, hipStream_t st);
int pad_c3_c4_launch(const float* in, int64_t npix, float* out, hipStream_t st);
int preprocess_u8_launch(const uint8_t* in, int N, int Hin, int Win, float* out, int Hout, int Wout, int Hpad, int Wpad, int64_t out_img_stride,
                         const float* mean3, const float* std3, int swap_rb, hipStream_t st, int hflip = 0);
// csrc/resample.hip: PIL-exact 8-bit bilinear resize of a batch in one launch (the arguments of isegmi_op_resample_u8)
int resample_u8_launch(const uint8_t* d_src, int64_t src_bytes, const int32_t* d_table, const int32_t* h_table, int N, const int32_t* d_coeffs,
                       int64_t coeff_words, float* d_out, int planes, int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3,
                       int swap_rb, float fill, uint8_t* d_out_u8, int64_t out_u8_bytes, hipStream_t st);
int pad_c3_c32_launch(const float* in, int64_t npix, float* out, hipStream_t st);
int yolact_detect_launch(const isegmi_yolact_detect_args* a, hipStream_t st);
// Detect in two halves: everything up to the final per-image top-k, then the gather.  coeff_sel (optional, [N][max_det][mask_dim] pre-tanh): the gather
// takes slot (n, q)'s coefficients from there instead of from d_mask.
int yolact_detect_select_launch(const isegmi_yolact_detect_args* a, hipStream_t st);
int yolact_detect_gather_launch(const isegmi_yolact_detect_args* a, const float* coeff_sel, hipStream_t st);
// the index rows the final top-k's flat indices refer to in the block's nms_mode: prior = idx[n * nc * K + flat]
int yolact_nms_status_launch(const int32_t* overflow, int N, int32_t* status, hipStream_t st);   // det.nms_overflow -> rle.status[3]
void yolact_detect_index_view(const isegmi_yolact_detect_args* a, const int32_t** idx, int* nc, int* K);
// yolact_coeff.hip: the coefficient rows of selected priors, bit-identical to the head convolution's outputs
struct CoeffLevels { const float* feat[5]; int H[5], W[5]; int n = 0; };
int yolact_coeff_index_launch(const int32_t* fin_idx, const int32_t* tk_idx, const int32_t* fin_cnt, int N, int nc, int top_k, int max_det, int A,
                              const CoeffLevels& lv, int32_t* rows, hipStream_t st);
int yolact_coeff_rows_launch(const CoeffLevels& lv, int N, int Cin, int R, int S, int pad, const float* w_packed, const float* scale, const float* shift,
                             int A, int row0, int mask_dim, const int32_t* rows, const int32_t* count, int max_det, float* out, hipStream_t st);
// csrc/vit_ops.hip (each header comment of include/isegmi.h states the contract)
int vit_attention_launch(const float* qkv, int N, int T, int heads, float* out, hipStream_t st);
int vit_layer_norm_launch(const float* x, int64_t rows, int D, int64_t x_stride, const float* gamma, const float* beta, float eps, float* out,
                          int64_t out_stride, hipStream_t st);
int vit_gelu_launch(const float* x, float* y, int64_t n, int gelu_tanh, hipStream_t st);
int vit_patchify_launch(const float* in, int N, int H, int W, int P, float* out, hipStream_t st);
int vit_softmax_launch(const float* x, int rows, int n, float* prob, hipStream_t st);
int yolact_masks_launch(const float* proto, const float* coeffs, const float* boxes, const int* count, int N, int PH, int PW,
                        int mask_dim, int K, int h, int w, float* ws_lo, uint8_t* out_masks, int64_t* out_boxes, hipStream_t st,
                        const int* image_hw = nullptr, int* win = nullptr, bool clear = true, bool dense_lo = false);

}  // namespace isegmi

struct isegmi_engine {
    isegmi::Engine e;
};
