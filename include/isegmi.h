/*
 * isegmi.h -- C ABI of libisegmi.so: the MI355X (gfx950) RoI/mask inference hot path of
 * detectron.jittor's Mask R-CNN and Yolact.jittor.
 *
 * Drop-in boundary.  The reference defines NO native / FFI / plugin interface for this path:
 * /root/reference holds only README.md (the submodules are empty) and the
 * only boundary it shows is the Python call surface
 *     COCODemo(cfg, min_image_size=800, confidence_threshold=0.5)      README.md:320-324
 *     coco_demo.run_on_opencv_image(image)                             README.md:331
 *     python eval.py --trained_model=... --score_threshold=... --top_k=...  README.md:243-249
 *     python tools/test_net.py --config-file ...                       README.md:344-347
 * Each entry point below names the reference operator it stands in for (SURVEY.md section 8a
 * ids M1..M13 / Y1..Y8 and Appendix A item) and the README line that reaches it.  The Python
 * package `isegmi` binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * negative code on failure, message via isegmi_last_error() (thread-local).  Pointers named
 * d_* are DEVICE pointers obtained from isegmi_malloc; h_* are host pointers.  All activations
 * are fp32 NHWC.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * A handle is single-stream and not thread-safe: one handle per GPU per process.
 */
#ifndef ISEGMI_H
#define ISEGMI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define ISEGMI_ABI_VERSION 1

int isegmi_version(void);
const char* isegmi_last_error(void);

/* ---- device plumbing (replaces `jt.flags.use_cuda = 1`, README.md:311) ---- */
int isegmi_device_count(int* n);
int isegmi_set_device(int device_id);
int isegmi_malloc(void** d_ptr, int64_t bytes);
int isegmi_free(void* d_ptr);
int isegmi_malloc_host(void** h_ptr, int64_t bytes);   /* pinned host memory (source of isegmi_engine_upload_async) */
int isegmi_free_host(void* h_ptr);
int isegmi_h2d(void* d_dst, const void* h_src, int64_t bytes);
int isegmi_d2h(void* h_dst, const void* d_src, int64_t bytes);
int isegmi_memset(void* d_ptr, int value, int64_t bytes);
int isegmi_sync(void);
/* Box calibration (diagnostic, not on the product path): what this device sustains on three bare loops of about ms_per_leg milliseconds each --
 * dependent v_mfma_f32_32x32x2_f32 and v_mfma_f32_32x32x16_f16 chains on random register operands (four waves per SIMD, no memory traffic) and a
 * float4 copy of 1 GiB (read + written bytes).  bench.py prints them as "box" so that a slow box can be told from a slow build (boxes of one pool
 * differ by 3-12 %: MI355X_MICROARCH.md "DVFS give-back" 5). */
int isegmi_box_calibrate(double ms_per_leg, double* mfma_f32_tflops, double* mfma_f16_tflops, double* hbm_copy_gbs);

/* ---- convolution family: M2 M3 M4 M8 M10 M11 Y2 Y3 Y4 Y5 ----
 * Implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 with fused per-channel affine
 * (folded BN or bias), residual add and activation.  Per output element the accumulation is
 * ONE fmaf chain from +0 over the R*S*Cin products, walked in groups of 128 input channels
 * (outermost), then (r, s), then the group's channels -- plain (r, s, cin) for Cin <= 128 and for
 * 1x1 convolutions -- bit-identical to the oracle (oracle/ora_ops.c, ora_conv2d). */
typedef struct isegmi_conv_desc {
    int32_t N, H, W, Cin;            /* input NHWC; Cin % 32 == 0, or Cin == 4 with R==S==7 (stem) */
    int32_t Cout, R, S, stride, pad;
    int32_t act;                     /* 0 none, 1 relu, 2 tanh, 3 LeakyReLU(0.1), 4 LeakyReLU(0.1) then + residual (DarkNet block); fp32 only for 2-4 */
    int32_t tile;                    /* 0 auto; fp32: 1: 128x128  2: 128x64  3: 64x64 (round-1 schedule; the stem)  4: 32x32 on 16x16x4 MFMA  5: 32x32 with four loader waves, software-pipelined  6: 32x64, two 16x16 tiles per wave (block tile MxN)
                                        10 / 12: 64x64, v2 schedule, loads 2 / 4 chunks ahead (the default for large grids)  7 / 9: the same with the early LDS store (measured slower; kept for A/B)
                                        13 / 14: hybrid launch -- v2 tiles (loads 2 / 4 ahead) on the rows that fill the CUs a whole number of times, 32x32 blocks on the left-over rows (the default for 513-2600-tile grids with a small left-over);
                                        15 (fp32, NEVER chosen by tile 0): FIXED-TREE SPLIT-K -- a 32x32 block whose K chunks are cut over four sets of waves, out = ((p0 + p1) + p2) + p3 of four
                                        k-ordered partial chains over the chunk ranges [q L, (q + 1) L), L = ceil(K / 32 / 4): an opt-in numerics mode (bit-exact against the oracle's
                                        ora_conv2d_split, NOT against isegmi_op_conv2d's other tiles) for the small-M, large-K layers of a bs = 1 forward; the engines' `conv_split_k`;
                                        fp16: 1: 256x256  2: 256x128  3: 128x128  4: 64x64  5: 64x128  6: 64x256  7: 128x256  8: 128x64  9: 192x256  10: 192x128  11: 160x256;
                                        12/13/14/16: 192x256, 256x256, 256x128, 160x256 with 4 loader waves, 17: 192x256 as 12 MFMA + 4 loader waves, 19: 128x256 + 4, 20: 192x128 as 6 + 2;
                                        26/27/28/29: row-strip kernel for 3x3/1/1 (192x256, 256x128, 160x256, 192x256 on 12 MFMA waves) with 4 loader waves; 30/31: 29/26 with three B chunk buffers;
                                        32/34/37/39: persistent forms of 12/14/17/19 (a block walks several tiles, the loader waves stream the next tile during the epilogue);
                                        + 2048 (test hook): persistent kernels on an 8-block grid */
    int32_t out_div;                 /* output pixels per "image" for addressing; 0 -> Ho*Wo */
    int64_t out_img_stride;          /* floats; 0 -> out_div*out_pix_stride */
    int64_t out_pix_stride;          /* floats; 0 -> Cout */
} isegmi_conv_desc;

int isegmi_conv_out_hw(const isegmi_conv_desc* d, int32_t* Ho, int32_t* Wo);
/* 1 when the split-K mode's shape rule takes this fp32 layer (at most 176 tiles of 64 x 64 and K >= 1024; not the stem), else 0.  The engines apply it, under
 * `conv_split_k`, to the bottleneck convolutions of the backbone except a stage's first conv1 / projection; the oracle models mirror it (oracle/ora.py). */
int isegmi_conv_split_qualifies(const isegmi_conv_desc* d);
/* number of floats of the packed weight image */
int isegmi_conv_packed_floats(const isegmi_conv_desc* d, int64_t* n);
/* host: natural [Cout][R][S][Cin] -> packed image consumed by isegmi_op_conv2d */
int isegmi_pack_conv_weights(const isegmi_conv_desc* d, const float* h_w_krsc, float* h_packed);
/* d_scale / d_shift / d_residual may be NULL (1 / 0 / none). residual is contiguous [M][Cout]. */
int isegmi_op_conv2d(const isegmi_conv_desc* d, const float* d_in, const float* d_wpacked,
                     const float* d_scale, const float* d_shift, const float* d_residual,
                     float* d_out, void* stream);
/* n <= 10 independent fp32 convolutions (no stem, tile 0) as ONE launch: the shared-weight heads of all FPN levels, the FPN's lateral / output convs.
 * Member i = descs[i] with d_in[i], d_w[i] (packed), d_scale[i] / d_shift[i] / d_res[i] (each array, or an entry, may be NULL), d_out[i]; every member's
 * result is bit-identical to its own isegmi_op_conv2d call -- same results, tile form chosen per GROUP (ring depth, 64 x 64 tiles or 32 x 32 blocks): every
 * fp32 tile form keeps one k-ordered chain per output.  The pointer arrays are HOST arrays; a NULL d_in[i] / d_w[i] / d_out[i] is ISEGMI_ERR_ARG. */
int isegmi_op_conv2d_group(int n, const isegmi_conv_desc* descs, const float* const* d_in, const float* const* d_w, const float* const* d_scale,
                           const float* const* d_shift, const float* const* d_res, float* const* d_out, void* stream);

/* Grouped 3x3 convolution (ResNeXt conv2: MODEL.RESNETS.NUM_GROUPS > 1) on v_mfma_f32_16x16x4_f32, fp32 NHWC.  The descriptor is isegmi_conv_desc as it
 * stands; `groups` rides next to it.  Supported: R = S = 3, pad 1, stride 1 or 2, Cin == Cout with Cin % 64 == 0, cg = Cin / groups in {8, 16, 32, 64},
 * act 0 or 1, a dense contiguous output (out_div / out_img_stride / out_pix_stride 0) and tile 0; anything else is ISEGMI_ERR_ARG and launches nothing.
 * N * Ho * Wo == 0 is a successful no-op.  Numerics: the fp32 contract of isegmi_op_conv2d per group -- output channel co of group g = co / cg is ONE chain
 * acc = fmaf(x_k, w_k, acc) from +0 over k = (r, s, c) ascending, c over the group's own input channels g cg .. g cg + cg - 1 (padding taps are x = 0
 * products), then y = fmaf(acc, scale, shift) + residual -> act.  An output depends on its own group's input channels only, non-finite values included.
 * groups == 1 with Cin == 64 equals isegmi_op_conv2d bit for bit.  h_w is [Cout][3][3][Cin / groups]; the packed image has as many floats as h_w. */
int isegmi_conv_grouped_packed_floats(const isegmi_conv_desc* d, int groups, int64_t* n);
int isegmi_pack_conv_weights_grouped(const isegmi_conv_desc* d, int groups, const float* h_w, float* h_packed);
int isegmi_op_conv2d_grouped(const isegmi_conv_desc* d, int groups, const float* d_in, const float* d_wpacked,
                             const float* d_scale, const float* d_shift, const float* d_residual,
                             float* d_out, void* stream);

/* fp16 variant (BASELINE configs[4]: "fp16 MFMA conv"): fp16 storage, v_mfma_f32_32x32x16_f16, fp32 accumulate
 * and epilogue.  Cin % 64 == 0 (or the stem, below); act none/relu; d_in / d_wpacked / d_residual are fp16, d_out fp16 or (out_f32)
 * fp32.  The 16-term sum inside one MFMA is not an ordered chain: parity with the oracle is tolerance-based. */
int isegmi_conv_packed_halfs(const isegmi_conv_desc* d, int64_t* n);
int isegmi_pack_conv_weights_f16(const isegmi_conv_desc* d, const float* h_w_krsc, uint16_t* h_packed);
int isegmi_op_conv2d_f16(const isegmi_conv_desc* d, const void* d_in, const void* d_wpacked,
                         const float* d_scale, const float* d_shift, const void* d_residual, void* d_out,
                         int out_f32, void* stream);
/* Fused identity bottleneck, fp16 (M2 `BottleneckWithFixedBatchNorm`, blocks 1.. of res2 / res3 under configs[4]):
 * out = relu(bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(x)))))))) + x) in ONE launch; the two Cmid-channel intermediates stay in LDS as
 * fp16 (rounded where the three-launch path rounds them when it stores them: results are bit-identical to three isegmi_op_conv2d_f16
 * calls with (r, s, cin)-ordered tiles), x is read once, out written once.  (Cin, Cmid) = (256, 64) or (512, 128); Cout = Cin = 4 Cmid;
 * weights are the isegmi_pack_conv_weights_f16 images of the three layers, scale / shift the folded FrozenBN of each. */
typedef struct isegmi_bottleneck_desc {
    int32_t N, H, W, Cin, Cmid;
    int32_t flags;                   /* bit 0 (test hook): 8-block grid, so that small shapes exercise the multi-tile stream; any other bit is rejected (ISEGMI_ERR_ARG) -- the
                                        timing-only experiment bits of the development builds (-DISEGMI_EXPERIMENT_FLAGS) produce wrong results and do not exist in a release build */
} isegmi_bottleneck_desc;
int isegmi_op_bottleneck_f16(const isegmi_bottleneck_desc* d, const void* d_x, const void* d_w1, const float* d_s1, const float* d_b1,
                             const void* d_w2, const float* d_s2, const float* d_b2, const void* d_w3, const float* d_s3,
                             const float* d_b3, void* d_out, void* stream);
/* The FIRST block of res2 (Cin = Cmid = 64, stride 1) with its projection shortcut d (1x1 64 -> 256 + BN) in the same launch:
 * out = relu(bn3(conv3(...)) + fp16(bnd(conv1x1_d(x)))) -- the shortcut tensor is rounded to fp16 where the four-launch path stores it. */
int isegmi_op_bottleneck_ds_f16(const isegmi_bottleneck_desc* d, const void* d_x, const void* d_w1, const float* d_s1, const float* d_b1,
                                const void* d_w2, const float* d_s2, const float* d_b2, const void* d_w3, const float* d_s3,
                                const float* d_b3, const void* d_wd, const float* d_sd, const float* d_bd, void* d_out, void* stream);
/* FPN top-down step under configs[4] (M3: `last_inner = inner_block(feature) + interpolate(last_inner, scale_factor=2, mode="nearest")`) as one launch: desc = the
 * lateral 1x1 / 1 / 0 conv (Cout % 8 == 0, W >= 8, tile 0), d_coarse = the coarser level [N][Hc][Wc][Cout] fp16; out = fp16(fp16(conv) + coarse[n][y/2][x/2]),
 * bit-identical to isegmi_op_conv2d_f16 followed by the engine's nearest-2x add (the lateral result is rounded to fp16 where that path stores it). */
int isegmi_op_conv1x1_up2x_add_f16(const isegmi_conv_desc* d, const void* d_in, const void* d_wpacked, const float* d_scale, const float* d_shift,
                                   const void* d_coarse, int Hc, int Wc, void* d_out, void* stream);
/* RPNHead under configs[4] (M4: `t = relu(conv3x3(x)); logits, deltas = cls_logits(t), bbox_pred(t)`) as one launch: desc = the 3x3 / 1 / 1 conv (Cout 256,
 * act 1, tile 0), d_w2packed / scale2 / shift2 = the fused cls + bbox 1x1 (256 -> cout2 <= 32 outputs, isegmi_pack_conv_weights_f16 image), d_out2 = fp32
 * [M][cout2].  t is rounded to fp16 where the two-launch path stores it and never leaves the CU; results are bit-identical to isegmi_op_conv2d_f16 twice.
 * *fused = 0 and NOTHING is launched when the layer is too small for the 192 x 256 row-strip tile the fusion lives on: the caller then runs the two launches. */
int isegmi_op_conv3x3_head_f16(const isegmi_conv_desc* d, const void* d_in, const void* d_wpacked, const float* d_scale, const float* d_shift,
                               const void* d_w2packed, const float* d_scale2, const float* d_shift2, int cout2, float* d_out2, int* fused, void* stream);
/* fp16 stem (M2 `StemWithFixedBatchNorm` conv1 under configs[4]): desc Cin=4 R=S=7 stride=2 pad=3 with H, W the image
 * size; d_in of isegmi_op_conv2d_f16 is then the haloed fp16 image [N][H+6][(W+7)&~1][4] this op writes from the fp32
 * NHWC C=3 batch (3 zero pixels on every side, zero 4th channel); weights are given as [Cout][7][7][4]. */
int isegmi_op_pad_c3_to_f16_halo(const float* d_in_nhwc3, int N, int H, int W, void* d_out, void* stream);
/* The whole stem in one launch (csrc/stem_pool_f16.hip): out = maxpool3x3/2/1(relu(bn(conv7x7/2/3(image)))) from the haloed image above, the packed
 * stem weights (isegmi_pack_conv_weights_f16 of the Cin=4 R=S=7 desc, Cout = 64) and the folded FrozenBN; d_out = [N][Hp][Wp][64] fp16 with
 * Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1.  Bit-identical to isegmi_op_conv2d_f16 (act 1) followed by the engine's fp16 max-pool (3, 2, 1; a max of fp16 values is exact);
 * the conv output stays in LDS.  flags (test hooks): bit 0: 8-block grid (blocks walk many units); bit 1: the shortest units (every seam between row segments). */
int isegmi_op_stem_pool_f16(int N, int H, int W, const void* d_halo, const void* d_w, const float* d_scale, const float* d_shift, void* d_out,
                            int flags, void* stream);

/* MFMA shape of the fp16 backbone tiles (process-wide tuning knob): 0: v_mfma_f32_32x32x16_f16 everywhere; 1: the 192 x 256 row-strip tile of the 3x3
 * layers and the fused RPN head on v_mfma_f32_16x16x32_f16 (same output tile per wave, same LDS images; the chip holds a higher clock on it in power-bound
 * loops: +8 % on the 634-GF layer); 2: 1 + the persistent 192 x 256 / 256 x 128 / 128 x 256 tiles and the UP2X merge (memory-bound: no gain); 3 (default):
 * 1 + the 144-row forms (48-row wave tiles, possible with 16 x 16 blocks only) for Cout <= 256 layers whose 192-row tiles leave CUs idle in one round.
 * RESULTS DO NOT DEPEND ON THE SHAPE: one 16 x 16 x 32 instruction sums its 32 products bit for bit as two chained 32 x 32 x 16 instructions do
 * (tools/microbench/mfma_shape.hip), so every fused-vs-unfused bit identity of the fp16 family holds under any setting.
 * conv tile ids 40 / 44 / 47 / 49 force the 16 x 16 x 32 form of 30 / 34 / 37 / 39 for one launch, 41 / 46 the 144-row forms of 40 / 47. */
int isegmi_set_f16_mfma_shape(int shape);
int isegmi_get_f16_mfma_shape(int* shape);

/* device front end (Y1 FastBaseTransform, README.md:243-249 `--image=...`; M1 build_transform + to_image_list, README.md:320-331): a uint8
 * [N][Hin][Win][3] batch -> fp32 NHWC3 [N][Hpad][Wpad][3]: bilinear (align_corners = False) to Hout x Wout (identity when the sizes match),
 * out[.., swap_rb ? 2-c : c] = (v[c] - mean3[c]) / std3[c], zeros in the padding; bit-identical to the oracle's ora_fast_base_transform /
 * ora_build_transform (oracle/ora_ops.c: the rounding sequence is stated there) and to the numpy transforms of isegmi/transforms.py */
int isegmi_op_preprocess_u8(const uint8_t* d_in, int N, int Hin, int Win, float* d_out, int Hout, int Wout, int Hpad, int Wpad,
                            int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, void* stream);
/* the same with one more argument (the mirrored views of TEST.BBOX_AUG): hflip != 0 preprocesses the image whose columns are reversed within
 * Win (not within the canvas: the image keeps its top-left corner, the padding stays right and bottom) -- bit-identical to isegmi_op_preprocess_u8 on a
 * host-flipped copy of the bytes, which therefore go up once for both views of a scale */
int isegmi_op_preprocess_u8_flip(const uint8_t* d_in, int N, int Hin, int Win, float* d_out, int Hout, int Wout, int Hpad, int Wpad,
                                 int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, int hflip, void* stream);

/* ---- PIL-exact 8-bit bilinear resampling (csrc/resample.hip) ----
 * The resize of the R-CNN front ends and of the YOLOv3 letterbox on the device, bit-identical to PIL's Image.resize(..., BILINEAR) on 8-bit images
 * (Resample.c: integer arithmetic over 22-bit fixed-point coefficient tables; horizontal pass first, rounded to bytes, then the vertical pass).
 *
 * isegmi_resample_coeffs: the tables of one axis I -> O, host only (no GPU needed), computed in double without contraction exactly as PIL does:
 * bounds [O][2] = (xmin, n), kk [O][ksize] (unused slots 0), *ksize = 2 ceil(max(I / O, 1)) + 1.  bounds = kk = NULL asks for *ksize alone.
 * Refuses I, O < 1 and scales whose ksize exceeds ISEGMI_RESAMPLE_MAX_KSIZE (downscales beyond 512; the ten contract shapes go up to 300). */
#define ISEGMI_RESAMPLE_MAX_KSIZE 1025
int isegmi_resample_coeffs(int I, int O, int32_t* bounds, int32_t* kk, int* ksize);
/* One image of a batch is one row of ISEGMI_RESAMPLE_ENTRY_WORDS int32 words in the image table:
 *   0, 1  byte offset of its [Hin][Win][3] uint8 pixels in d_src (low, high word of an int64; any alignment)
 *   2..5  Hin, Win, Hout, Wout            6, 7  dst_y, dst_x: where the resized image sits on the canvas (fp32 output only)
 *   8, 9  word offsets in d_coeffs of the horizontal (Win -> Wout) and vertical (Hin -> Hout) tables, each laid out bounds [O][2] then kk [O][ksize]
 *   10, 11 their ksize                    12  hflip: output column x shows column Wout - 1 - x of the RESIZED image
 *   13    the canvas plane it is written to (fp32 output)      14, 15  byte offset of its tight [Hout][Wout][3] output in d_out_u8 (int64) */
#define ISEGMI_RESAMPLE_ENTRY_WORDS 16
/* One launch for the whole batch.  d_table is the DEVICE table; h_table the same rows on the host, which this call validates against src_bytes,
 * coeff_words and the output before it launches (the kernel additionally clamps every table bound to its image).  Exactly one output:
 *   d_out != NULL: planes fp32 NHWC3 canvases of Hpad x Wpad, out_img_stride floats apart: out[.., swap_rb ? 2 - c : c] = ((float)p - mean3[c]) / std3[c]
 *                  inside the image, `fill` everywhere else on the canvas of every plane a row names (each canvas element written exactly once);
 *   d_out_u8 != NULL: the resized bytes, tight, at each row's output offset (Hpad, Wpad, mean3, std3, swap_rb, fill unused). */
int isegmi_op_resample_u8(const uint8_t* d_src, int64_t src_bytes, const int32_t* d_table, const int32_t* h_table, int N, const int32_t* d_coeffs,
                          int64_t coeff_words, float* d_out, int planes, int Hpad, int Wpad, int64_t out_img_stride, const float* mean3,
                          const float* std3, int swap_rb, float fill, uint8_t* d_out_u8, int64_t out_u8_bytes, void* stream);
/* the kernel's output tile (rows, columns) and the source rows one LDS chunk holds: the sizes its tests straddle */
int isegmi_op_resample_tile(int* tile_h, int* tile_w, int* chunk_rows);

/* max_pool2d(k,s,p), -inf padding (M2/Y2 stem; k=1,s=2 = LastLevelMaxPool M3) */
int isegmi_op_maxpool(const float* d_in, int N, int H, int W, int C, int k, int s, int p,
                      float* d_out, void* stream);
/* bilinear align_corners=False to (Ho,Wo), optional +add, optional relu (Y3, Y4) */
int isegmi_op_resize_bilinear(const float* d_in, int N, int H, int W, int C, int Ho, int Wo,
                              const float* d_add, int relu, float* d_out, void* stream);
/* Keypoint R-CNN predictor tail ([UPSTREAM-RECALL] KeypointRCNNPredictor): d_in [R][Hi][Wi][4*K] is ConvTranspose2d(4, 2, 1) run as a 3x3
 * convolution with parity-major outputs (channel (2 py + px) * K + k belongs to pixel (2y + py, 2x + px)); d_out [R][4 Hi][4 Wi][K] = bilinear x2
 * (align_corners False) of that pixel shuffle, bit-identical to shuffling on the host and calling isegmi_op_resize_bilinear. */
int isegmi_op_keypoint_heatmap(const float* d_in, int64_t R, int Hi, int Wi, int K, float* d_out, void* stream);
/* Keypointer / heatmaps_to_keypoints on the device, one launch, the resized maps never exist in memory: for detection slot (n, c) with c < d_count[n] and box
 * (x1, y1, x2, y2) = d_boxes[n][c]: w = max(x2 - x1, 1), wc = ceil(w) (h likewise); each of the K maps d_heat[n * cap + c][S][S][k] is resized bicubically
 * (A = -0.75, half-pixel centres, clamped taps, horizontal pass first, every product and sum a separate fp32 operation) to hc x wc; the first maximum in
 * row-major order at (x_int, y_int) gives d_kpt[n][c][k] = ((x_int + 0.5) * (w / wc) + x1, (y_int + 0.5) * (h / hc) + y1, 1) and d_kscore[n][c][k] = the
 * resized value there.  Slots c >= d_count[n] are written as zeros and their maps are not read.  S <= 64, K <= 32, N * cap <= 65535; resized sides are
 * cut at 16384.  NaN maps are outside the contract. */
int isegmi_op_keypoint_decode(const float* d_heat, const float* d_boxes, const int32_t* d_count, int N, int cap, int S, int K, float* d_kpt,
                              float* d_kscore, void* stream);
/* modulated deformable im2col: the sampling stage of the DCNv2 3x3 convolutions of the YOLACT++ backbones
 * (the YOLACT++ rows of README.md:216-221).  d_offset_mask [N][Ho][Wo][3*R*S] is the raw conv_offset_mask
 * output (channel 2k = dy_k, 2k+1 = dx_k, 2*R*S+k = mask logit); d_out [N][Ho][Wo][R*S][C] feeds a 1x1
 * convolution over R*S*C channels with the layer's KRSC weights.  C % 4 == 0. */
int isegmi_op_deform_im2col(const float* d_x, int N, int H, int W, int C, const float* d_offset_mask,
                            int R, int S, int stride, int pad, int dil, float* d_out, void* stream);
/* the DCNv1 form of isegmi_op_deform_im2col (the `dconv` models of maskrcnn-benchmark's dcn/ configs): d_offset [N][Ho][Wo][2*R*S] holds the offsets
 * alone (channel 2k = dy_k, 2k+1 = dx_k) and no mask factor is applied.  Equal, bit for bit, to the modulated entry fed a saturated mask logit. */
int isegmi_op_deform_im2col_v1(const float* d_x, int N, int H, int W, int C, const float* d_offset,
                               int R, int S, int stride, int pad, int dil, float* d_out, void* stream);
/* Fused 3x3 deformable convolution, fp32 NHWC: pad 1, dilation 1, stride 1 or 2; the columns of isegmi_op_deform_im2col are sampled
 * straight into the MFMA operand tile and never written.  d_om [N][Ho][Wo][OC] is the raw output of the offset convolution: modulated 1 (DCNv2), OC = 27,
 * channel 2k = dy_k, 2k+1 = dx_k, 18+k = mask logit; modulated 0 (DCNv1), OC = 18.  d_w is the isegmi_pack_conv_weights image of the 1x1 descriptor over
 * 9*C input channels ([Cout][3][3][C] weights), d_scale / d_shift / d_res optional, act 0 or 1.  The result d_out [N][Ho][Wo][Cout] is bit-identical to
 * isegmi_op_deform_im2col (or _v1) followed by isegmi_op_conv2d as that 1x1: one chain per output, taps outermost, the C channels of a tap ascending.
 * C % 32 == 0, 32 <= C <= 512, Cout % 4 == 0; anything else is ISEGMI_ERR_ARG and launches nothing.  N*Ho*Wo == 0 is a successful no-op. */
int isegmi_op_deform_conv2d(const float* d_x, int N, int H, int W, int C, const float* d_om, int OC, int modulated, int stride,
                            const float* d_w, int Cout, const float* d_scale, const float* d_shift, const float* d_res, int act, float* d_out,
                            void* stream);
/* out = lateral + nearest2x(coarse) (M3) */
int isegmi_op_upsample_nearest2x_add(const float* d_coarse, int N, int Hc, int Wc, int C,
                                     const float* d_lateral, int H, int W, float* d_out,
                                     void* stream);
/* GroupNorm over NHWC fp32 ([UPSTREAM-RECALL] maskrcnn-benchmark group_norm(): torch.nn.GroupNorm(groups, C, eps, affine=True)):
 *   out = (x - mu) * rsqrt(var + eps) * gamma + beta [+ residual] [ReLU], mu / biased var over (H, W, C / groups) of one image (or RoI) and one group.
 * N images or RoI slabs (N == 0 launches nothing).  C % 4 == 0, groups divides C, and a 64-channel tile holds whole groups (C % 64 == 0 and
 * 64 % (C / groups) == 0, or C < 64).  d_residual (x's shape) is optional; d_out may be d_x (in place).  Planes of H * W <= 196 run as one launch
 * with the slab in registers; larger planes run statistics + apply passes and need d_workspace of isegmi_op_group_norm_workspace_bytes() bytes
 * (0 for the small planes, where d_workspace may be NULL).  No atomics, fixed summation order (csrc/groupnorm.hip): same input, same bits. */
int64_t isegmi_op_group_norm_workspace_bytes(int64_t N, int H, int W, int C, int groups);
int isegmi_op_group_norm(const float* d_x, int64_t N, int H, int W, int C, int groups, const float* d_gamma, const float* d_beta, float eps,
                         const float* d_residual, int relu, float* d_out, void* d_workspace, int64_t workspace_bytes, void* stream);
/* NHWC3 -> NHWC4 zero pad (stem input) */
int isegmi_op_pad_c3_to_c4(const float* d_in, int64_t npix, float* d_out, void* stream);
/* fn: 0 exp 1 sigmoid 2 tanh 3 log2 -- exposes the deterministic math for parity tests */
int isegmi_op_map_f32(const float* d_x, float* d_y, int64_t n, int fn, void* stream);
/* fp16-storage twins of isegmi_op_maxpool / _resize_bilinear / _upsample_nearest2x_add (configs[4]) -- exposes the kernels of csrc/spatial_f16.hip
 * for parity tests.  Tensors are fp16 NHWC (d_in of the max-pool is fp32 when in_f16 == 0); all arithmetic is fp32 in the order of the fp32 ops, only
 * loads and stores convert: out = fp16(op(fp32(in))).  C % 4 == 0; the max-pool's output (H + 2p - k) / s + 1 must not be empty. */
int isegmi_op_maxpool_f16(const void* d_in, int in_f16, int N, int H, int W, int C, int k, int s, int p, void* d_out, void* stream);
int isegmi_op_resize_bilinear_f16(const void* d_in, int N, int H, int W, int C, int Ho, int Wo, const void* d_add, int relu, void* d_out, void* stream);
int isegmi_op_upsample_nearest2x_add_f16(const void* d_coarse, int N, int Hc, int Wc, int C, const void* d_lateral, int H, int W, void* d_out,
                                         void* stream);

/* ---- selection: torch.topk / sort stand-in (M6, M9, Y6) ----
 * rows independent problems; row r = d_keys + r*row_stride, n elements; output sorted by
 * (score desc, index asc); k <= 8192.  k_eff = min(k, n, d_limit[r / rows_per_limit]) when
 * d_limit != NULL.  d_vals/d_idx are [rows][k]; d_cnt [rows] (optional) receives k_eff.
 * Key order contract: keys compare as floats -- -0.0 and +0.0 are equal (the lower index first, as torch.topk / sort
 * order them), +-inf and subnormals are ordinary keys.  d_vals holds the selected keys bit for bit, except that a
 * selected -0.0 is returned as +0.0 (both zeros share one sort key).  NaN keys are outside the contract. */
int isegmi_op_topk(const float* d_keys, int64_t row_stride, int rows, int n, int k,
                   const int32_t* d_limit, int rows_per_limit, float* d_vals, int32_t* d_idx,
                   int32_t* d_cnt, void* stream);

/* ---- Yolact Detect (Y6; App. A.6/A.9; README.md:243 --top_k / --score_threshold path) ----
 * softmax -> decode -> conf prefilter -> per-class top_k -> fast-NMS -> per-image top max_det.
 * d_conf holds LOGITS [N][P][ncls]; d_loc [N][P][4]; d_mask [N][P][mask_dim] (tanh applied);
 * d_priors [P][4] (cx,cy,w,h).  Outputs are fixed-capacity [N][max_det]. */
typedef struct isegmi_yolact_detect_args {
    int32_t N, P, ncls, mask_dim, top_k, max_det;
    float conf_thresh, nms_thresh;
    const float* d_conf;
    const float* d_loc;
    const float* d_mask;
    const float* d_priors;
    /* workspace (caller-allocated device memory) */
    float* d_ws_scoresT;     /* [N][ncls-1][P] */
    float* d_ws_boxes;       /* [N][P][4] decoded xyxy (relative) */
    int32_t* d_ws_counts;    /* [2N] */
    float* d_ws_tk_vals;     /* [N][ncls-1][top_k] */
    int32_t* d_ws_tk_idx;    /* [N][ncls-1][top_k] */
    int32_t* d_ws_tk_cnt;    /* [N][ncls-1] */
    float* d_ws_cand;        /* [N][ncls-1][top_k] */
    float* d_ws_fin_vals;    /* [N][max_det] */
    int32_t* d_ws_fin_idx;   /* [N][max_det] */
    int32_t* d_ws_fin_cnt;   /* [N] */
    /* outputs */
    int32_t* d_out_count;    /* [N] */
    float* d_out_boxes;      /* [N][max_det][4] relative xyxy */
    float* d_out_scores;     /* [N][max_det] */
    int32_t* d_out_classes;  /* [N][max_det] 0..ncls-2 */
    float* d_out_coeffs;     /* [N][max_det][mask_dim] */
    int32_t* d_out_prior;    /* [N][max_det] */
    /* optional fused-head layout (all zero = the three contiguous buffers above): the prediction head was run as ONE
     * convolution whose per-pixel output row holds [A x 4 loc | A x ncls conf | A x mask_dim mask]; then d_conf, d_loc
     * and d_mask all point at that buffer [N][P/A][pix_stride] and prior p = pix*A + a reads from row pix.
     * mask_tanh: the mask block holds pre-activation values; tanh is applied to the <= max_det gathered rows. */
    int32_t A;
    int32_t mask_tanh;
    int64_t pix_stride;
    int32_t off_loc, off_conf, off_mask;
    int32_t second_threshold;   /* App. A.6 fork, fast_nms(second_threshold=True): a box must also have its class score > conf_thresh (a prior passes
                                   the pre-filter on its BEST class and is ranked in every class); 0 = the default detect() call */
    /* suppression rule (every field from here on may stay zero: nms_mode 0 is the path above, launch for launch).
     *   1  cross-class fast NMS (upstream cc_fast_nms): score = max_c prob[c], class = the lowest c attaining it, ONE top_k and one fast-NMS pass per image;
     *      the survivors are cut to the best max_det.  Needs d_ws_cc_scores / d_ws_cc_class; d_ws_tk_* and d_ws_cand are used as [N][top_k].
     *   2  traditional NMS (upstream traditional_nms + cython_nms): per class the priors with prob[c] > conf_thresh in (score desc, prior asc) order,
     *      greedy, boxes * trad_scale, legacy +1 areas, suppress on ovr >= nms_thresh; at most trad_cap candidates per (image, class) are visited.
     *      d_ws_tk_vals / d_ws_tk_idx are then [N][ncls-1][trad_cap] and d_ws_cand [N][ncls-1][128] (a class's first 128 survivors: no later one can
     *      enter the cut, max_det <= 128); top_k is not used.  Needs d_ws_trad_list and d_ws_trad_prior.
     * second_threshold != 0 next to nms_mode 1 or 2 is refused. */
    int32_t nms_mode;
    int32_t trad_cap;            /* mode 2: a multiple of 64 in [64, 2048]; 0 = 1024 */
    float trad_scale;            /* mode 2: upstream's cfg.max_size (> 0) */
    int32_t* d_out_nms_total;    /* [N], optional, every mode: survivors of the suppression pass before the cut to max_det */
    int32_t* d_out_nms_overflow; /* [N], optional: 1 iff (mode 2) some class of the image held more than trad_cap candidates AND fewer than max_det of
                                    its first trad_cap survived -- the only case in which the cap can change the result; 0 in modes 0 and 1 */
    float* d_ws_cc_scores;       /* mode 1: [N][P] */
    int32_t* d_ws_cc_class;      /* mode 1: [N][P] */
    int32_t* d_ws_trad_list;     /* mode 2: [1 + N*(ncls-1)] */
    int32_t* d_ws_trad_prior;    /* mode 2: [N][ncls-1][128] */
} isegmi_yolact_detect_args;
int isegmi_op_yolact_detect(const isegmi_yolact_detect_args* a, void* stream);

/* ---- Yolact mask coefficients of selected priors (the engines' `lazy_coeffs`: the forward runs the loc | conf rows of the fused prediction head
 * only, and the 32 coefficients of the <= max_det kept detections per image are computed after the final top-k) ----
 * d_feats[l] (l < nlevels <= 5; a HOST array of device pointers): the head's input map of level l, [N][Hs[l]][Ws[l]][Cin] fp32.  d_wpacked / d_scale /
 * d_shift: a packed stride-1 R x S fp32 layer (isegmi_pack_conv_weights) with at least row0 + 32 A output channels.  d_rows [N][max_det][5] int32:
 * slot (n, q) = (image, level, ho, wo, anchor); d_count [N]: valid slots of image n.  d_out [N][max_det][32]: for slot (n, q), q < count[n],
 * out[j] = the layer's output channel row0 + 32 anchor + j at pixel (ho, wo) of that image and level, with act 0 -- bit for bit what isegmi_op_conv2d
 * stores there (the same k-ordered fmaf chain and epilogue), pre-tanh.  Slots past the count, and slots whose row is out of range (a negative level
 * marks one), are NOT written. */
int isegmi_op_yolact_coeff_rows(int nlevels, const float* const* d_feats, const int32_t* Hs, const int32_t* Ws, int N, int Cin, int R, int S,
                                int pad, const float* d_wpacked, const float* d_scale, const float* d_shift, int A, int row0,
                                const int32_t* d_rows, const int32_t* d_count, int max_det, float* d_out, void* stream);

/* ---- Yolact postprocess masks (Y7; App. A.9) ----
 * d_proto [N][PH][PW][32]; d_coeffs [N][K][32]; d_boxes [N][K][4] relative; d_count [N].
 * d_ws_lo [N][K][PH][PW] fp32 workspace (holds the crop windows' pixels of the proto-resolution masks afterwards, the rest is
 * undefined); d_out_masks [N][K][h][w] uint8 {0,1} (only the first
 * count[n] masks of image n are written); d_out_boxes [N][K][4] int64 (may be NULL). */
int isegmi_op_yolact_masks(const float* d_proto, const float* d_coeffs, const float* d_boxes,
                           const int32_t* d_count, int N, int PH, int PW, int mask_dim, int K, int h,
                           int w, float* d_ws_lo, uint8_t* d_out_masks, int64_t* d_out_boxes,
                           void* stream);
/* The same stage with the forks the engines take (parity-test entry).  d_image_hw [N][2] (may be NULL): image n is assembled at its own (h_n, w_n)
 * in the top-left corner of the common h x w plane.  d_win [N][K][4] (may be NULL) receives, for every slot below the count, a window
 * (x0, y0, x1, y1) that holds every set pixel of the slot; slots past the count are not written.  clear = 0: the planes are not zeroed first and only
 * the bytes inside each window are written (a reader goes through the windows).  dense_lo = 1: d_ws_lo receives the complete zero-padded
 * proto-resolution masks of the slots below the count, not only their crop windows' pixels. */
int isegmi_op_yolact_masks_win(const float* d_proto, const float* d_coeffs, const float* d_boxes, const int32_t* d_count, int N, int PH, int PW,
                               int mask_dim, int K, int h, int w, float* d_ws_lo, uint8_t* d_out_masks, int64_t* d_out_boxes,
                               const int32_t* d_image_hw, int32_t* d_win, int clear, int dense_lo, void* stream);
/* YOLACT++ mask re-scoring, first layer (parity-test entry): d_lo [NK][PH][PW] -> d_out [NK][Ho][Wo][32], Ho = (PH - 3) / 2 + 1, Wo = (PW - 3) / 2 + 1:
 * channels 0..7 = relu(3x3 stride-2 conv with d_w [8][9], d_b [8]; nine chained fmaf, then the bias), channels 8..31 = 0.  PH, PW >= 3. */
int isegmi_op_maskiou_conv1(const float* d_lo, int NK, int PH, int PW, const float* d_w, const float* d_b, float* d_out, void* stream);
/* YOLACT++ mask re-scoring, last step (parity-test entry): d_feat [N*K][HW][C], d_cls / d_score [N][K], d_count [N] ->
 * d_out [n][d] = d_score[n][d] * max over HW of d_feat[n*K + d][.][d_cls[n][d]] for d < d_count[n], else 0. */
int isegmi_op_maskiou_rescore(const float* d_feat, int N, int K, int HW, int C, const int32_t* d_cls, const float* d_score, const int32_t* d_count,
                              float* d_out, void* stream);

/* ---- Mask R-CNN RoI ops (M6 M7 M9 M10 M11 M12; App. A.4-A.8; all reached from README.md:331) ---- */
/* Semantic forks of the NMS (which of them detectron.jittor takes is unknown -- the reference tree holds no code -- so every one is a
 * switch).  OR-ed into the `nms_flags` argument of isegmi_op_rpn_level / _rpn_levels / isegmi_box_post_args; 0 = maskrcnn-benchmark's CUDA path. */
#define ISEGMI_NMS_GE 1           /* suppress on iou >= thr (the CPU loop) instead of iou > thr (the CUDA kernel, jt.nms) */
#define ISEGMI_NMS_NO_PLUS_ONE 2  /* plain areas (x2-x1)*(y2-y1) in the IoU instead of the legacy +1 widths */
#define ISEGMI_NMS_INDEX_ORDER 4  /* box post-processing only: a class's kept detections in ascending proposal index (the CPU NMS returns nonzero(keep))
                                     instead of score order; the RPN truncates a score-sorted list, where both orders keep the same boxes in the same order */
/* greedy NMS (A.6): `problems` independent sets of n <= 6144 boxes; visiting order (score desc, index
 * asc); IoU with legacy +1 areas when plus_one; suppress on iou > thr (ge: >=).  d_keep [problems][n]
 * receives ORIGINAL indices in score order, d_cnt [problems] the count (<= max_keep when max_keep > 0).
 * Scores follow isegmi_op_topk's key order contract: -0.0 == +0.0 (index decides), no NaN. */
int isegmi_op_nms(const float* d_boxes, const float* d_scores, int problems, int n, float thr,
                  int plus_one, int ge, int max_keep, int32_t* d_keep, int32_t* d_cnt, void* stream);
/* LevelMapper + RoIAlign (A.7).  aligned 0: the legacy op (no half-pixel shift, RoI at least one pixel wide and high -- maskrcnn-benchmark); aligned 1:
 * ROIAlign(aligned=True) -- scaled corners minus 0.5, no minimum size (the other side of the App. A.7 fork).  d_feats: host array of nlevels device pointers
 * (NHWC, level k_min first); rois [N][K][4] image coords; counts [N]; out [N*K][PH][PW][C] (rows past
 * count zero-filled).  fixed_level >= 0 bypasses the LevelMapper.  d_out_level [N][K] optional.
 * sampling > 0: fixed sampling x sampling grid per bin; sampling <= 0: adaptive ceil(roi / pooled) (ROIAlign's
 * sampling_ratio = 0, used by the R-50-C4 config of README.md:263-273). */
int isegmi_op_roi_align(const float* const* d_feats, const int32_t* Hs, const int32_t* Ws,
                        const float* scales, int nlevels, const float* d_rois, const int32_t* d_counts,
                        int N, int K, int C, int PH, int PW, int sampling, int aligned, int k_min, int fixed_level,
                        float* d_out, int32_t* d_out_level, void* stream);
/* nn.AvgPool2d over the whole window of every RoI (FastRCNNPredictor of the C4 box head): x [R][HW][C] -> out [R][C] */
int isegmi_op_avgpool_full(const float* d_x, int64_t R, int HW, int C, float* d_out, void* stream);
/* fp16-storage LevelMapper + RoIAlign (configs[4]): d_feats / d_out are fp16, arithmetic is the fp32 op's. */
int isegmi_op_roi_align_f16(const void* const* d_feats, const int32_t* Hs, const int32_t* Ws,
                            const float* scales, int nlevels, const float* d_rois, const int32_t* d_counts,
                            int N, int K, int C, int PH, int PW, int sampling, int aligned, int k_min, void* d_out, void* stream);
/* The FPN heads' RoIAlign (sampling 2, LevelMapper) as two launches.  isegmi_op_roi_prep, one thread per RoI: d_table [N*K][2*(PH+PW)+1][4]
 * int32 -- for each of the RoI's 2*PH sample rows and 2*PW sample columns {byte offset of the low tap, of the high tap, weight of the low
 * tap, of the high tap (fp32 bits)} with the validity test and clamps of the scalar op applied (a sample outside the map: weights +0 and tap offsets
 * past the end of the map, which the pooling launch's range-checked loads read as 0), then {level index, H, W, signature of (C * elem_bytes, PH, PW)} -- and, when
 * d_order is not NULL, d_order [N][K] = every image's RoI rows n*K + k sorted by (level, Morton code of the RoI centre on that level's map),
 * rows past count last.  K <= 2048; elem_bytes 4 (fp32 features) or 2 (fp16); a level's map must stay under 512 MiB per image; `aligned` as in isegmi_op_roi_align.
 * isegmi_op_roi_align_ordered / _f16_ordered then run workgroup L on one 128-byte channel slice of RoI d_order[L / 8 ...] (d_order NULL: row
 * order) so that RoIs sharing pixels are in flight together and every XCD's L2 holds its own slice of them; 7x7 or 14x14 bins, C in
 * {32..256} (fp32) / {64..512} (fp16).  Outputs are those of isegmi_op_roi_align / _f16 bit for bit for ANY feature values (inf / NaN included), whatever
 * permutation d_order holds (entries outside [0, N*K) are skipped, rows it leaves out are not written).  d_rois / d_counts / scales / k_min must be the
 * ones the table was made from; a table made for another C * elem_bytes / PH / PW fills the RoI's output with NaN. */
int64_t isegmi_op_roi_table_bytes(int N, int K, int PH, int PW);
int isegmi_op_roi_prep(const float* d_rois, const int32_t* d_counts, int N, int K, const int32_t* Hs, const int32_t* Ws,
                       const float* scales, int nlevels, int k_min, int C, int PH, int PW, int elem_bytes, int aligned,
                       int32_t* d_order, void* d_table, void* stream);
int isegmi_op_roi_align_ordered(const float* const* d_feats, const int32_t* Hs, const int32_t* Ws,
                                const float* scales, int nlevels, const float* d_rois, const int32_t* d_counts,
                                const int32_t* d_order, const void* d_table, int N, int K, int C, int PH, int PW,
                                int k_min, float* d_out, void* stream);
int isegmi_op_roi_align_f16_ordered(const void* const* d_feats, const int32_t* Hs, const int32_t* Ws,
                                    const float* scales, int nlevels, const float* d_rois, const int32_t* d_counts,
                                    const int32_t* d_order, const void* d_table, int N, int K, int C, int PH, int PW,
                                    int k_min, void* d_out, void* stream);
/* PostProcessor.filter_results (A.5): softmax, per-class decode(10,10,5,5)+clip, score filter, NMS,
 * kth-value cut to det_per_img.  Output order: class ascending, NMS (score) order inside a class -- proposal-index order with
 * ISEGMI_NMS_INDEX_ORDER. */
typedef struct isegmi_box_post_args {
    int32_t N, R, ncls, det_per_img, cap, nms_flags;   /* nms_flags: OR of ISEGMI_NMS_* */
    float score_thresh, nms_thresh;
    int64_t logits_stride, regr_stride;   /* floats between consecutive rois */
    const float* d_logits;     /* [N*R] rows of ncls */
    const float* d_regr;       /* [N*R] rows; class j deltas at 4j..4j+3 (cls_agnostic: 4..7 for every class) */
    const float* d_props;      /* [N][R][4] */
    const int32_t* d_prop_cnt; /* [N] */
    const int32_t* d_image_hw; /* [N][2] unpadded (h, w) */
    float* d_ws_prob;          /* [N][R][ncls] */
    float* d_ws_cand_scores;   /* [N][ncls-1][R] */
    float* d_ws_cand_boxes;    /* [N][ncls-1][R][4] */
    int32_t* d_ws_kept_total;  /* [N] */
    float* d_ws_top_vals;      /* [N][det_per_img] */
    int32_t* d_ws_top_idx;     /* [N][det_per_img] */
    int32_t* d_out_count;      /* [N] */
    float* d_out_boxes;        /* [N][cap][4] */
    float* d_out_scores;       /* [N][cap] */
    int32_t* d_out_labels;     /* [N][cap] 1..ncls-1 (0 = empty) */
    /* optional (all four or none): classes with more than 128 candidates get their suppression matrix from the whole chip (three launches instead of
     * one block per class building it alone: ~85 us for a 1000-candidate class); same kept lists */
    void* d_ws_crowd_matrix;     /* [N][ncls-1] x 131072 bytes */
    void* d_ws_crowd_keys;       /* [N][ncls-1][R] 8-byte keys */
    float* d_ws_crowd_boxes;     /* [N][ncls-1][R][4] */
    int32_t* d_ws_crowd_m;       /* [N][ncls-1] */
    /* MODEL.CLS_AGNOSTIC_BBOX_REG: d_regr rows hold eight deltas and EVERY class decodes the last four (4..7), once per proposal in effect; 0 = per-class
     * deltas.  Appended last: a caller that zeroes the struct (required) keeps the per-class behaviour. */
    int32_t cls_agnostic;
} isegmi_box_post_args;
int isegmi_op_box_postprocess(const isegmi_box_post_args* a, void* stream);
/* mask predictor tail (A.8): out[r,p] = sigmoid(<feat[r,p,:], w[label_r,:]> + b[label_r]); label 0 -> zeros */
int isegmi_op_mask_logits_select(const float* d_feat, int R, int HW, int C, const float* d_w,
                                 const float* d_b, const int32_t* d_labels, float* d_out, void* stream);
/* the same tail on fp16 features (configs[4]; d_w, d_b and d_out stay fp32) -- exposes mask_logits_select_f16_launch for parity tests.  C % 4 == 0.
 * C == 256 with 16-byte aligned features takes the coalesced form, whose dot product is 8 chained FMAs per lane and a 32-lane butterfly (parity
 * with the fp32 op by tolerance); every other C sums in the fp32 op's order (same bits).  label <= 0 -> zeros. */
int isegmi_op_mask_logits_select_f16(const void* d_feat, int R, int HW, int C, const float* d_w, const float* d_b, const int32_t* d_labels,
                                     float* d_out, void* stream);
/* Masker(threshold, padding=1) paste (A.8): masks [N][K][M][M], boxes [N][K][4] -> u8 [N][K][im_h][im_w] */
int isegmi_op_paste_masks(const float* d_masks, const float* d_boxes, const int32_t* d_counts, int N,
                          int K, int M, int im_h, int im_w, float thr, uint8_t* d_out, void* stream);
/* The same paste with the forks the engines take (parity-test entry).  d_win [N][K][4] (may be NULL) receives, for every slot below the count, the
 * window (x0, y0, x1, y1) of the padded box clamped to the image: every set pixel lies inside it (x1 <= x0 or y1 <= y0: none is set); slots past
 * the count are not written.  clear = 0: the planes are not zeroed first; every byte inside a window is written, and outside it at most the three
 * bytes that share a 4-byte word with a window row's end (as zeros). */
int isegmi_op_paste_masks_win(const float* d_masks, const float* d_boxes, const int32_t* d_counts, int N, int K, int M, int im_h, int im_w,
                              float thr, uint8_t* d_out, int32_t* d_win, int clear, void* stream);
/* AnchorGenerator.grid_anchors (M5, A.3): d_out [(y*grid_w + x)*A + a][4] = d_base[a] + (x, y, x, y) * stride */
int isegmi_op_grid_anchors(const float* d_base, int A, int stride, int grid_h, int grid_w, float* d_out, void* stream);
/* one RPN level (A.4) for N images: fused head [N][HW][A*5] (A logits then A*4 deltas per pixel) */
int isegmi_op_rpn_level(const float* d_head, const float* d_anchors, const int32_t* d_image_hw, int N,
                        int HW, int A, int pre_nms, int post_nms, float nms_thr, float min_size,
                        int nms_flags /* ISEGMI_NMS_GE | ISEGMI_NMS_NO_PLUS_ONE */, float* d_ws_prob, float* d_ws_tk_vals, int32_t* d_ws_tk_idx,
                        int32_t* d_ws_tk_cnt, float* d_out_boxes, float* d_out_scores,
                        int32_t* d_out_cnt, void* d_ws_nms /* optional: N * 131072 bytes, the suppression
                        matrix of the chip-wide NMS used when pre_nms <= 1024; NULL = single-block NMS */,
                        void* stream);
/* the same for nl <= 5 FPN levels at once (SURVEY 2.1 "level x image as one batch dimension"): five launches -- sigmoid, two-level top-k, suppression
 * matrix, greedy scan -- over all (level, image) rows; 256 < pre_nms <= 1024.  d_heads / d_anchors: HOST arrays of nl DEVICE pointers ([N][HW_l][A*5] /
 * [HW_l*A][4]).  Outputs [N][nl][post_nms][4], [N][nl][post_nms] (-1 beyond the count), [N][nl]: level l's list is what isegmi_op_rpn_level gives for it,
 * bit for bit.  Workspaces (isegmi_op_rpn_levels_workspace): prob prob_elems floats, cand_vals / cand_idx cand_elems each, tk_vals / tk_idx
 * nl*N*pre_nms, tk_cnt nl*N, nms nl*N*131072 bytes. */
int isegmi_op_rpn_levels_workspace(int nl, int N, const int32_t* HW, int A, int pre_nms, int64_t* prob_elems, int64_t* cand_elems);
int isegmi_op_rpn_levels(int nl, const float* const* d_heads, const float* const* d_anchors, const int32_t* HW, const int32_t* d_image_hw, int N, int A,
                         int pre_nms, int post_nms, float nms_thr, float min_size, int nms_flags, float* d_ws_prob, float* d_ws_cand_vals,
                         int32_t* d_ws_cand_idx, float* d_ws_tk_vals, int32_t* d_ws_tk_idx, int32_t* d_ws_tk_cnt, void* d_ws_nms,
                         float* d_out_boxes, float* d_out_scores, int32_t* d_out_cnt, void* stream);

/* ---- RetinaNet tail ([UPSTREAM-RECALL] maskrcnn-benchmark RetinaNetPostProcessor, reached from README.md:344-347 with the retinanet configs) ----
 * isegmi_op_retina_select: forward_for_single_feature_map for nl <= 5 levels x N images in two launches.  Row (level l, image n) is d_logits[l] + n * HW[l]*A*C,
 * the cls_logits output as the convolution wrote it: flat index ((y*W + x)*A + a)*C + c.  p = dm_sigmoid(logit) (isegmi_op_map_f32 fn 1); candidates are
 * p > score_thresh (strict); the min(#candidates, top_n) best are kept, top_n <= 1024, ordered (p desc, flat index asc) -- isegmi_op_topk's key order contract on
 * the SIGMOID values (two logits may share one).  Every logit is read once; no probability tensor is written; exact for any number of candidates; bitwise
 * reproducible.  NaN logits are outside the contract.  d_sel_scores / d_sel_idx [N][nl][top_n] (-1 past the count), d_sel_cnt [N][nl].
 * Decode (d_out_boxes != NULL; then d_deltas[l] [N][HW_l][A*4], d_anchors[l] [HW_l*A][4] and d_image_hw [N][2] (h, w) are read): anchor = idx / C, label =
 * idx % C + 1, BoxCoder(10, 10, 5, 5) with the legacy +1 widths and the log(1000/16) clamp, clip to (w - 1, h - 1), boxes with a side (+1) under min_size
 * dropped, selection order kept.  d_out_boxes [N][nl*top_n][4], d_out_scores / d_out_labels [N][nl*top_n] (level l's list starts at l*top_n; -1 / 0 past its
 * count), d_out_cnt [N][nl].  d_ws: isegmi_op_retina_select_workspace bytes (one list of top_n 8-byte keys per 8192 logits of every row; -1: bad sizes). */
#define ISEGMI_RETINA_MAX_LEVELS 5
typedef struct isegmi_retina_select_args {
    int32_t nl, N, A, C, top_n;
    float score_thresh, min_size;
    int32_t HW[ISEGMI_RETINA_MAX_LEVELS];
    const float* d_logits[ISEGMI_RETINA_MAX_LEVELS];
    const float* d_deltas[ISEGMI_RETINA_MAX_LEVELS];
    const float* d_anchors[ISEGMI_RETINA_MAX_LEVELS];
    const int32_t* d_image_hw;
    void* d_ws;
    int64_t ws_bytes;
    float* d_sel_scores;
    int32_t* d_sel_idx;
    int32_t* d_sel_cnt;
    float* d_out_boxes;
    float* d_out_scores;
    int32_t* d_out_labels;
    int32_t* d_out_cnt;
} isegmi_retina_select_args;
int64_t isegmi_op_retina_select_workspace(int nl, int N, const int32_t* HW, int A, int C, int top_n);
int isegmi_op_retina_select(const isegmi_retina_select_args* a, void* stream);
/* isegmi_op_retina_postprocess: select_over_all_levels.  Per image nseg lists of seg_len candidate slots (nseg * seg_len <= 8192), the first d_seg_cnt[n][s] of
 * list s valid -- isegmi_op_retina_select's decode outputs with nseg = nl, seg_len = top_n; a label outside 1..ncls-1 drops its slot.  For every class greedy NMS
 * over the class's candidates in (score desc, slot asc) order, IoU and threshold as isegmi_op_nms under nms_flags (a box never meets a box of another class: no
 * coordinate offsets); kept lists concatenated in class order, NMS order inside a class -- slot order with ISEGMI_NMS_INDEX_ORDER; when more than det_per_img > 0
 * remain, those with score >= the det_per_img-th largest stay; at most cap rows.  Any distribution over the classes, one class may hold every slot.
 * Outputs as isegmi_box_post_args': d_out_count [N], d_out_boxes [N][cap][4], d_out_scores [N][cap], d_out_labels [N][cap] (zeros past the count). */
typedef struct isegmi_retina_post_args {
    int32_t N, nseg, seg_len, ncls, det_per_img, cap, nms_flags;
    float nms_thresh;
    const float* d_boxes;        /* [N][nseg*seg_len][4] */
    const float* d_scores;       /* [N][nseg*seg_len] */
    const int32_t* d_labels;     /* [N][nseg*seg_len] */
    const int32_t* d_seg_cnt;    /* [N][nseg] */
    void* d_ws;                  /* isegmi_op_retina_postprocess_workspace(N, nseg, seg_len) bytes (-1: bad sizes) */
    int64_t ws_bytes;
    int32_t* d_out_count;
    float* d_out_boxes;
    float* d_out_scores;
    int32_t* d_out_labels;
} isegmi_retina_post_args;
int64_t isegmi_op_retina_postprocess_workspace(int N, int nseg, int seg_len);
int isegmi_op_retina_postprocess(const isegmi_retina_post_args* a, void* stream);
/* ---- test-time box augmentation ([UPSTREAM-RECALL] maskrcnn-benchmark engine/bbox_aug.py, unverified) ----
 * isegmi_op_bbox_aug_candidates: one view's raw box-predictor output -> candidates of the per-image pool, in the first view's coordinates.  Inputs in
 * isegmi_box_post_args' layout, passed flat.  For every proposal row r < d_prop_cnt[n] (rows at or past the count are never read) and class j = 1..ncls-1 with
 * p = softmax(logits[r])[j] > score_thresh (strict; the bits of isegmi_op_box_postprocess' probability tensor): box = clip(decode(props[r], deltas[r, j])) as
 * in isegmi_op_box_postprocess (BoxCoder(10, 10, 5, 5), legacy +1, log(1000/16) clamp, clip to (w - 1, h - 1) of d_image_hw; cls_agnostic: deltas 4..7 for
 * every class); hflip: x1' = w - x2 - 1, x2' = w - x1 - 1 in fp32; then x *= d_ratios_wh[n][0], y *= d_ratios_wh[n][1] (one fp32 multiplication each).
 * Candidates are appended to the pool in (proposal asc, class asc) order behind the d_pool_cnt[n] entries already there: slot s < cap gets
 * d_pool_boxes[n][s], d_pool_scores[n][s] = p, d_pool_labels[n][s] = j; d_pool_cnt[n] advances to min(cap, old + found), d_pool_total[n] by found -- the
 * pool holds the first cap candidates and total > cap is the overflow signal.  Two launches, no atomics, bitwise reproducible.  R <= 1024, ncls 2..256,
 * cap 1..8192; bad sizes return ISEGMI_ERR_ARG before any launch.  The merge is isegmi_op_retina_postprocess with nseg 1, seg_len cap, d_seg_cnt d_pool_cnt. */
int64_t isegmi_op_bbox_aug_workspace(int N, int R);   /* bytes of d_ws (-1: bad sizes) */
int isegmi_op_bbox_aug_candidates(int N, int R, int ncls, int cls_agnostic, int hflip, int cap, float score_thresh,
                                  const float* d_logits /* [N*R] rows of ncls */, int64_t logits_stride /* floats between consecutive rois */,
                                  const float* d_regr /* [N*R] rows; class j deltas at 4j..4j+3 (cls_agnostic: 4..7) */, int64_t regr_stride,
                                  const float* d_props /* [N][R][4] */, const int32_t* d_prop_cnt /* [N] */,
                                  const int32_t* d_image_hw /* [N][2] the VIEW's unpadded (h, w) */,
                                  const float* d_ratios_wh /* [N][2] (w0 / w_view, h0 / h_view) as float */, void* d_ws, int64_t ws_bytes,
                                  float* d_pool_boxes /* [N][cap][4] */, float* d_pool_scores /* [N][cap] */, int32_t* d_pool_labels /* [N][cap] */,
                                  int32_t* d_pool_cnt /* [N] read, then advanced */, int32_t* d_pool_total /* [N] the uncapped running count */,
                                  void* stream);
/* ---- YOLOv3 tail and route ([UPSTREAM-RECALL] the public yolov3.cfg, unverified) ----
 * isegmi_op_yolo_select: objectness x class selection, top-n cut and grid decode for nl <= 3 levels x N images in two launches, straight from the raw head
 * tensors.  d_heads[l] is [N][H_l][W_l][A * (5 + C)] as the convolution wrote it, channel a * (5 + C) + k, k = 0..4 = tx, ty, tw, th, to, then the class logits;
 * grid_hw [nl][2] = (H_l, W_l), strides [nl], anchors_wh [nl][A][2] in pixels: host arrays.  A (cell, anchor, class) is a candidate iff s = sigmoid(to) *
 * sigmoid(t_c) > conf_thresh (strict; multi_label 0: only the class of the largest sigmoid, lowest index on ties).  Per (level, image) the min(#candidates,
 * top_n) best by (s desc, flat index ((y W + x) A + a) C + c asc) are decoded -- bx = (sigmoid(tx) + x) stride, bw = exp(tw) anchor_w, corners bx -+ bw / 2,
 * clipped to [0, canvas_w] x [0, canvas_h]; a NaN box and a box with a side below min_wh are dropped -- into isegmi_op_retina_postprocess's input layout:
 * d_out_boxes [N][nl * top_n][4], d_out_scores / d_out_labels [N][nl * top_n] (label c + 1; rows past a count: zero box, score -1, label 0), d_out_cnt [N][nl],
 * and d_out_total [N][nl] = the candidates BEFORE the top_n cut.  A 1..8, C 1..256, top_n 1..1024, conf_thresh >= 0.  d_ws: isegmi_op_yolo_select_workspace
 * bytes (-1: bad sizes).  isegmi_op_yolo_slice_records: the anchor records one block of the first launch takes for class count C. */
#define ISEGMI_YOLO_MAX_LEVELS 3
int isegmi_op_yolo_slice_records(int C);
int64_t isegmi_op_yolo_select_workspace(int nl, int N, const int32_t* grid_hw, int A, int C, int top_n);
int isegmi_op_yolo_select(int nl, int N, const float* const* d_heads, const int32_t* grid_hw, const int32_t* strides, const float* anchors_wh, int A, int C,
                          int top_n, float conf_thresh, int multi_label, float min_wh, int canvas_w, int canvas_h, void* d_ws, int64_t ws_bytes,
                          float* d_out_boxes, float* d_out_scores, int32_t* d_out_labels, int32_t* d_out_cnt, int32_t* d_out_total, void* stream);
/* darknet's upsample + route: d_out [N][2 Hc][2 Wc][Cc + Cs] = [d_coarse[n][y / 2][x / 2] | d_skip[n][y][x]]; Cc, Cs multiples of 32.  NULL pointers and
 * sizes <= 0 are refused before any launch. */
int isegmi_op_concat_up2x(const float* d_coarse, int N, int Hc, int Wc, int Cc, const float* d_skip, int Cs, float* d_out, void* stream);
/* darknet's [maxpool] (csrc/yolo_pool.hip), NHWC fp32: d_out [N][(H - 1) / stride + 1][(W - 1) / stride + 1][C]; the window of output o
 * starts at o * stride - (size - 1) / 2 (integer divisions: an even size pads on the bottom / right only).  zero_pad 0: taps outside the map are skipped
 * (darknet); 1: each contributes +0.0f (ZeroPad2d + MaxPool2d of the PyTorch ports).  The maximum is isegmi_op_maxpool's (v > m ? v : m from -inf: the
 * largest non-NaN tap, -inf where there is none); with zero_pad 0, stride 1 and an odd size the result is bit-identical to isegmi_op_maxpool(size, 1,
 * size / 2).  C % 4 == 0, size 1..13, stride 1..2; NULL pointers and sizes outside these sets are refused before any launch. */
int isegmi_op_maxpool_darknet(const float* d_in, int N, int H, int W, int C, int size, int stride, int zero_pad, float* d_out, void* stream);
/* The SPP block of yolov3-spp as one launch: d_out [N][H][W][4 C] = [mp13 | mp9 | mp5 | d_in] (route layers = -1, -3, -5, -6), mpK =
 * isegmi_op_maxpool_darknet(size K, stride 1, zero_pad) as values.  C % 32 == 0, H and W 1..32; anything else is refused before any launch. */
int isegmi_op_spp_concat(const float* d_in, int N, int H, int W, int C, int zero_pad, float* d_out, void* stream);

/* ---- ViT operators (csrc/vit_ops.hip states every operation order, tests/vit_ref.py restates it).  fp32, finite inputs only: NaN and
 * inf are outside these contracts.  Pointers 16-byte aligned.
 * isegmi_op_attention: softmax(q k^T / 8) v per (image, head), head dimension 64.  d_qkv [N][T][3 * heads * 64] as the qkv projection wrote it: channel
 * which * D + h * 64 + d (which 0 q, 1 k, 2 v; D = heads * 64) belongs to head h; d_out [N][T][D], head h at channels h * 64 ..  1 <= T <= 1024.
 *   s_ij = (fmaf chain from +0 over d ascending of q_i[d] k_j[d]) * 0.125;  m_i = max_j s_ij;  e_ij = dm_exp(s_ij - m_i);
 *   l_i = (c_0 + c_1) + (c_2 + c_3) with c_r the chain from +0 of e_ij over j = r, r + 4, ... ascending;  p_ij = e_ij / l_i (IEEE division);
 *   o_i[d] = fmaf chain from +0 over j ascending of p_ij v_j[d].  Tokens past T are never read. */
int isegmi_op_attention(const float* d_qkv, int N, int T, int heads, float* d_out, void* stream);
/* LayerNorm over the last axis: row r = d_x + r * x_row_stride, D floats (D % 4 == 0, D <= 2048; strides in floats, multiples of 4);
 * y = ((x - x[0]) - m) * rstd * gamma + beta with m / rstd from fp32 per-lane chains of the shifted data folded in fp64 (biased variance, clamped at 0);
 * d_out may be d_x.  The same bits for the same row whatever the row count or the strides. */
int isegmi_op_layer_norm(const float* d_x, int64_t rows, int D, int64_t x_row_stride, const float* d_gamma, const float* d_beta, float eps,
                         float* d_out, int64_t out_row_stride, void* stream);
/* GELU, elementwise, d_y may be d_x.  gelu_tanh 0: (0.5 x) * (1 + erf(x * fp32(1 / sqrt 2))), erf = Cephes erff / erfcf with every operation rounded on
 * its own; 1: (0.5 x) * (1 + tanh(fp32(sqrt(2 / pi)) * (x + 0.044715 * ((x * x) * x)))). */
int isegmi_op_gelu(const float* d_x, float* d_y, int64_t n, int gelu_tanh, void* stream);
/* [N][H][W][3] -> [N][H / P][W / P][P * P * 3], element (py * P + px) * 3 + c of a patch = its pixel (py, px), channel c: the patch embedding then is a
 * 1x1 convolution over P * P * 3 channels.  H and W multiples of P. */
int isegmi_op_patchify(const float* d_in_nhwc3, int N, int H, int W, int P, float* d_out, void* stream);
/* softmax of `rows` rows of n logits: e_j = dm_exp(x_j - max); lane l of 64 chains e_l + e_(l + 64) + ... from +0, the lane sums fold as the tree
 * s[l] += s[l + off], off = 32 .. 1; prob_j = e_j / sum (IEEE division). */
int isegmi_op_class_softmax(const float* d_logits, int rows, int n, float* d_prob, void* stream);

/* ---- the painter (csrc/render.hip): mask tints, box outlines and keypoint dots of a draw list on a uint8 image, bit for bit what the
 * host overlays do (COCODemo.overlay / overlay_keypoints, cli._overlay; the annotated image README.md:243-249 and the Detectron example end in) ----
 * d_image / d_out [H][W][3] u8, dense, the caller's channel order; d_out == d_image paints in place.  d_masks [slots][ph][pw] u8 planes with the image in
 * their top-left H x W (det.masks), a byte != 0 is set.  d_entries i32 [D][8] = {slot (-1: no mask), x1, y1, x2, y2, colour = c0 | c1 << 8 | c2 << 16,
 * flags (bit 0: outline), 0}, D <= 1024; d_dots i32 [Q][4] = {x, y, colour, half}, Q <= 32768, half 0..8.  Every pixel (x, y), every channel byte:
 *   for k = 0 .. D-1:  mask of entry k set here -> p = (p + c) >> 1;   outline flag and ((y1 <= y <= y2 and (x == x1 or x == x2)) or
 *                      (x1 <= x <= x2 and (y == y1 or y == y2))) -> p = c;          then for j = 0 .. Q-1:  |x - xj| <= half and |y - yj| <= half -> p = c.
 * Everything is a device pointer (a list may be NULL when its count is 0; d_masks NULL: box-only lists).  ISEGMI_ERR_ARG, with nothing launched or
 * written: a null image, H or W < 1, masks with slots < 1 or ph < H or pw < W, a slot outside -1 .. slots-1 or naming a slot without masks, D or Q over
 * its cap, half outside 0..8 (the lists are read back to the host and checked first: this entry point synchronises `stream`). */
int isegmi_op_paint(const uint8_t* d_image, int H, int W, const uint8_t* d_masks, int slots, int ph, int pw, const int32_t* d_entries, int D,
                    const int32_t* d_dots, int Q, uint8_t* d_out, void* stream);

/* ---- COCO run-length encoding on the device (the on-disk format behind inference() / tools/test_net.py,
 * README.md:344-347, annotation layout README.md:55-66; Yolact eval.py Detections.add_mask / dump, README.md:243-249) ----
 * pycocotools rleEncode + rleToString restated: for every valid slot (n, k), k < d_count[n], of the uint8 planes d_masks [N][K][plane_h][plane_w]
 * the column-major run lengths of the top-left (h_n, w_n) window (d_image_hw [N][2], NULL = the whole plane), starting with the run of
 * zeros, and their compressed ASCII string.  Slot m = n*K + k owns runs d_out_counts[d_out_run_off[m] .. d_out_run_off[m+1]) and characters
 * d_out_chars[d_out_str_off[m] .. d_out_str_off[m+1]); invalid slots own nothing.  d_out_status [4] = {total runs, total chars,
 * overflow bits (1: runs > cap_runs, 2: chars > cap_chars; the outputs are then incomplete), 0}.  Bit-identical to isegmi/coco.py
 * rle_counts / rle_to_string.  Workspace sizes: isegmi_rle_workspace. */
typedef struct isegmi_rle_args {
    int32_t N, K, plane_h, plane_w;
    int32_t cap_runs;                 /* entries of d_out_counts / d_ws_starts / d_ws_len: a multiple of 1024 */
    int32_t cap_chars;                /* bytes of d_out_chars */
    const uint8_t* d_masks;
    const int32_t* d_count;           /* [N] or NULL (all K slots valid) */
    const int32_t* d_image_hw;        /* [N][2] or NULL */
    const int32_t* d_windows;         /* [N*K][4] (x0, y0, x1, y1) or NULL: every set pixel of slot m lies inside [x0, x1) x [y0, y1); only that part
                                         of a plane is then read (pixels outside a window need not even be initialised) */
    void* d_ws_trans;                 /* workspace, sizes from isegmi_rle_workspace */
    int32_t* d_ws_col;
    int32_t* d_ws_nruns;
    int32_t* d_ws_tile;
    uint8_t* d_ws_len;
    uint32_t* d_ws_starts;
    int32_t* d_out_run_off;           /* [N*K + 1] */
    uint32_t* d_out_counts;           /* [cap_runs] */
    int32_t* d_out_str_off;           /* [N*K + 1] */
    uint8_t* d_out_chars;             /* [cap_chars] */
    int32_t* d_out_status;            /* [4] */
} isegmi_rle_args;
int isegmi_rle_workspace(int N, int K, int plane_h, int plane_w, int cap_runs, int64_t* trans_bytes, int64_t* col_bytes,
                         int64_t* nruns_bytes, int64_t* tile_bytes, int64_t* len_bytes, int64_t* starts_bytes);
int isegmi_op_rle_encode(const isegmi_rle_args* a, void* stream);

/* ---- Pose2Seg pose-guided stages (csrc/pose2seg_ops.hip) ----
 * Sizes are the model's: a 512 x 512 input, P2 = 128 x 128, 64 x 64 RoIs.  Keypoints are COCO's 17 (x, y, v) per person; instance r
 * belongs to image d_roi_img[r].  All warps share one bilinear helper (zero padding, taps
 * ((v00 wx0 + v01 wx1) wy0) + ((v10 wx0 + v11 wx1) wy1)); results are bit-identical to tests/pose2seg_ref.py. */
typedef struct isegmi_p2s_image {
    int64_t offset;                  /* byte offset of the image's [h][w][3] uint8 pixels in d_u8 */
    int32_t h, w;
    float minv[6];                   /* m1^-1 (input plane -> image pixels), row-major 2 x 3 */
    int32_t reserved[2];
} isegmi_p2s_image;
/* input letterbox (m1): d_out [N][S][S][4] = ((warp(v) / 255 - mean3[c]) / std3[c], ..., 0), v of channel swap_rb ? 2 - c : c; round_u8:
 * the warped value is rounded to u8 first (floor(v + 0.5) clamped to [0, 255]).  d_table [N] is a DEVICE array. */
int isegmi_op_pose2seg_letterbox(const uint8_t* d_u8, const isegmi_p2s_image* d_table, int N, int S, const float* mean3, const float* std3,
                                 int swap_rb, int round_u8, float* d_out, void* stream);
/* pose template fit, fp64: d_kpts [R][17][3] image pixels, d_m1 [N][6] the images' letterbox matrices, d_templates [T][17][3] (x, y, weight)
 * in align-frame pixels, T <= 64.  Outputs: d_m3 / d_G / d_mmask [R][6] fp32 (feature -> align, the pixel-space Affine-Align sampler matrix,
 * image -> output), d_kalign [R][17][3] (keypoints in the align frame, v copied), d_fit [R][8] fp64 = (m3, error, template index or -1 for
 * the fallback). */
int isegmi_op_pose2seg_fit(const float* d_kpts, const int32_t* d_roi_img, int R, const double* d_m1, const float* d_templates, int T,
                           int align_corners, float* d_m3, float* d_G, float* d_mmask, float* d_kalign, double* d_fit, void* stream);
/* Affine-Align: d_feat [N][Hf][Wf][C] -> channels [0, C) of d_out [R][64][64][out_c]; C % 4 == 0 */
int isegmi_op_pose2seg_align(const float* d_feat, int Hf, int Wf, int C, const int32_t* d_roi_img, const float* d_G, int R, float* d_out,
                             int out_c, void* stream);
/* skeleton features of d_kalign: channels [c0, c0 + 55) of d_out [R][64][64][out_c] (17 heatmaps, 19 limb vectors), zeros in
 * [c0 + 55, c0 + 64); out_c == c0 + 64 */
int isegmi_op_pose2seg_skeleton(const float* d_kalign, int R, float* d_out, int out_c, int c0, void* stream);
/* softmax of d_logits [R][64][64][2] and the reverse warp of channel 1 at d_mmask: d_masks [N][K][Hmax][Wmax] u8 = p > 0.5 for slot (n, k),
 * k < d_counts[n] (instance d_roi_off[n] + k), inside the image's own d_image_hw[n]; zeros elsewhere.  d_boxes [N][K][4] the tight xyxy box
 * (right / bottom exclusive; an empty mask: zeros), d_scores = 1, d_labels = 1 on valid slots (0 elsewhere), d_count_out = d_counts.
 * d_ws_box: [N][K][4] int32 workspace. */
int isegmi_op_pose2seg_masks(const float* d_logits, const float* d_mmask, const int32_t* d_counts, const int32_t* d_roi_off,
                             const int32_t* d_image_hw, int N, int K, int Hmax, int Wmax, int32_t* d_ws_box, uint8_t* d_masks, float* d_boxes,
                             float* d_scores, int32_t* d_labels, int32_t* d_count_out, void* stream);

/* ---- Keypoint R-CNN -> Pose2Seg hand-off (csrc/pose_handoff.hip) ----
 * One launch, one workgroup per image, all pointers DEVICE memory in the Keypoint R-CNN engine's layouts: d_score [N][cap], d_count [N], d_kpt
 * [N][cap][NK][3] in network-input coordinates, d_kscore [N][cap][NK], d_ratios_wh [N][2] = (ratio_w, ratio_h) as isegmi_engine_pack_keypoint_records takes
 * them.  A slot j < d_count[n] is a candidate when score > person_thresh (strict); the min(#candidates, K) best are kept, by score descending, equal scores
 * by slot ascending -- the input need not be sorted, a surplus is cut.  Keypoint k of a kept person becomes (x * ratio_w, y * ratio_h, v), one fp32
 * multiplication each, v = 2 when kscore > kp_thresh (strict), else 0.  Outputs: d_kpts_out [R][17][3] compact, image by image (image n's rows start at
 * the sum of d_count_out[m], m < n; room for N * K rows), d_score_out [N][K] (0 in unused slots), d_src_slot [N][K] int32 (the detection slot a person
 * came from, -1 unused), d_count_out [N].  The layout does not depend on execution order.  NK must be 17 (ISEGMI_ERR_ARG naming num_keypoints);
 * cap <= 4096; N * K <= 65535.  NaN scores are outside the contract. */
int isegmi_op_pose_handoff(const float* d_score, const int32_t* d_count, const float* d_kpt, const float* d_kscore, const float* d_ratios_wh, int N,
                           int cap, int NK, float person_thresh, float kp_thresh, int K, float* d_kpts_out, float* d_score_out, int32_t* d_src_slot,
                           int32_t* d_count_out, void* stream);
/* d_scores_out [N][K] takes d_scores_in [N][K] in the slots k < d_counts[n]; the other slots are left alone */
int isegmi_op_pose_scores(const float* d_scores_in, const int32_t* d_counts, int N, int K, float* d_scores_out, void* stream);

/* ---- model engine ----
 * Replaces the model object the reference builds inside COCODemo(cfg, ...) (README.md:320-324)
 * and Yolact eval.py (README.md:243): weights are pushed per layer under their upstream
 * state-dict names with BN already folded to (scale, shift) by the Python host; activations,
 * workspaces and outputs live in named device buffers owned by the engine. */
typedef struct isegmi_engine isegmi_engine;
/* model_kind: 1 = Yolact R50-FPN, 2 = Mask R-CNN R50/R101-FPN, 3 = Pose2Seg (H = W = 512), 4 = RetinaNet R50/R101-FPN, 5 = YOLOv3 (Darknet-53),
 * 7 = ViT classifier (6 is not assigned and is refused).  H, W = network input size. */
int isegmi_engine_create(int model_kind, int max_batch, int H, int W, isegmi_engine** out);
int isegmi_engine_destroy(isegmi_engine* e);
int isegmi_engine_set_param(isegmi_engine* e, const char* name, float value);
/* The value isegmi_engine_set_param last gave `name` on this engine; *is_set = 1 then, else 0 and *value = default_value (the caller states the default it
 * cares about: the engine's own defaults live where each parameter is read). */
int isegmi_engine_get_param(isegmi_engine* e, const char* name, float default_value, float* value, int32_t* is_set);
/* "graph" param != 0: a forward (yolact / maskrcnn) runs eagerly once, is captured into a hipGraph on the next call with the
 * same (batch, input pointer) and replayed afterwards (latency mode: ends joined on the main stream; any set_param /
 * set_conv / set_tensor drops the captured graphs).  Counters for tests and diagnostics: */
int isegmi_engine_graph_stats(isegmi_engine* h, int64_t* captures, int64_t* replays, int64_t* failures);
/* h_w_krsc: natural [Cout][R][S][Cin]; h_scale / h_shift [Cout] or NULL */
int isegmi_engine_set_conv(isegmi_engine* e, const char* name, int Cout, int R, int S, int Cin,
                           const float* h_w_krsc, const float* h_scale, const float* h_shift);
/* A grouped 3x3 layer (ResNeXt conv2; isegmi_op_conv2d_grouped): Cin == Cout, h_w [Cout][3][3][Cout / groups], groups > 1.  The layer carries its group
 * count: the trunk launches the grouped kernel for it, sizes the bottleneck buffers from the weights, never takes `conv_split_k` for it and counts its
 * grouped FLOPs in the timing records.  fp32 Mask R-CNN (FPN bodies) and RetinaNet engines; an fp16 engine, a C4 body and (at the forward) GroupNorm
 * weights next to a grouped layer are refused by name. */
int isegmi_engine_set_conv_grouped(isegmi_engine* e, const char* name, int Cout, int groups, const float* h_w, const float* h_scale, const float* h_shift);
/* constant tensors (priors, anchors, deconv weights ...) */
int isegmi_engine_set_tensor(isegmi_engine* e, const char* name, const void* h_data, int64_t bytes);
/* Yolact.forward (Y2-Y6): d_images NHWC3 fp32 [N][H][W][3] already normalised (Y1). Asynchronous
 * on the engine stream; results in buffers det.count/box/score/class/coeff/prior and proto. */
int isegmi_yolact_forward(isegmi_engine* e, const float* d_images_nhwc3, int N);
/* GeneralizedRCNN.forward (M2-M11): d_images NHWC3 fp32 [N][H][W][3], normalised and zero-padded to the
 * engine's (H,W); h_image_hw [N][2] = unpadded (h,w).  Results: det.count/box/score/label [N][cap],
 * det.mask28 [N][cap][28][28], proposals, rpn.* ... in named buffers. */
int isegmi_maskrcnn_forward(isegmi_engine* e, const float* d_images_nhwc3, const int32_t* h_image_hw, int N);
/* The same on a padded canvas (H, W) <= the engine's (H, W): d_images is [N][H][W][3] contiguous.  upstream's to_image_list pads every
 * BATCH to its own size (max over its images, rounded up to SIZE_DIVISIBILITY), so one engine -- weights packed once, buffers sized once
 * for the largest canvas -- serves every batch of a data set (COCODemo / inference(), README.md:320-331, 344-347).  The host sets the
 * per-level base anchors as tensors "anchor_base.<l>" [A][4] and the strides as params "anchor_stride<l>"; the grid is laid out on the
 * device for the current canvas (isegmi_op_grid_anchors). */
int isegmi_maskrcnn_forward_canvas(isegmi_engine* e, const float* d_images_nhwc3, const int32_t* h_image_hw, int N, int H, int W);
/* Test-time box augmentation (TEST.BBOX_AUG) on a box-only FPN engine: begin, one aug_view per view (the first one is view 0, whose
 * coordinates the results are in), merge.  aug_begin zeroes the pool counters aug.pool_cnt / aug.pool_total [N] and sizes aug.pool_box / _score / _label
 * for pool_cap (64..8192) slots per image.  aug_view runs the forward on that canvas up to and including the box predictor, then
 * isegmi_op_bbox_aug_candidates on its output: h_image_hw the view's sizes, hflip whether its input was mirrored, h_ratios_wh [N][2] = (w0 / w_view,
 * h0 / h_view) as float.  aug_merge runs isegmi_op_retina_postprocess over the pool into det.count / det.box / det.score / det.label (the plain forward's
 * buffers and order), leaves aug.pool_total fetchable (> pool_cap: the pool overflowed, the caller must not use det.*) and makes view 0's image sizes
 * current again.  fp32, mask_on 0, keypoint_on 0, no hipGraph, not the C4 body, at most 256 classes: everything else is refused by name.  A plain
 * forward before or after such a sequence behaves as ever. */
int isegmi_maskrcnn_aug_begin(isegmi_engine* e, int N, int pool_cap);
int isegmi_maskrcnn_aug_view(isegmi_engine* e, const float* d_images_nhwc3, const int32_t* h_image_hw, int N, int H, int W, int hflip,
                             const float* h_ratios_wh);
int isegmi_maskrcnn_aug_merge(isegmi_engine* e);
/* RetinaNet (model_kind 4; reached from tools/test_net.py with configs/retinanet_R-*-FPN_1x.yaml, README.md:344-347): the same calling form as
 * the Mask R-CNN pair -- d_images [N][H][W][3] zero-padded to a multiple of 32, h_image_hw [N][2] unpadded (h, w), one engine for every canvas up to its (H, W),
 * anchors ("anchor_base.<l>" [9][4], "anchor_stride<l>", l = 0..4 for P3..P7) laid out again when the canvas changes.  Results: det.count [N], det.box
 * [N][cap][4], det.score / det.label [N][cap] (cap = max(detections_per_img, detections_cap)); P3..P7, retina.logits<l> / retina.deltas<l>, retina.sel_score /
 * retina.sel_idx [N][5][top_n] with retina.sel_cnt [N][5], retina.cand_* in named buffers.  Params: retina_pre_nms_top_n (<= 1024), retina_inference_th,
 * retina_nms_th, retina_num_convs, detections_per_img, detections_cap, resnet_depth, nms_ge / nms_plus_one / nms_index_order.  fp32 only: "fp16" and "graph"
 * are refused by name, and so is a "retina_levels" other than 5. */
int isegmi_retinanet_forward(isegmi_engine* e, const float* d_images_nhwc3, const int32_t* h_image_hw, int N);
int isegmi_retinanet_forward_canvas(isegmi_engine* e, const float* d_images_nhwc3, const int32_t* h_image_hw, int N, int H, int W);
/* YOLOv3 (model_kind 5): d_images [N][H][W][3] = the letterboxed canvas of the engine's (H, W) (multiples of 32 in 32..1024), RGB, x / 255.
 * Darknet-53 -> three heads (head.<s>.conv0..6, head.<s>.route, s = 0 at stride 32) -> isegmi_op_yolo_select -> isegmi_op_retina_postprocess.  Results in
 * canvas coordinates: det.count [N], det.box [N][cap][4], det.score / det.label [N][cap]; yolo.head<s> (raw head tensors), yolo.cand_* and yolo.cand_cnt /
 * yolo.cand_total [N][3] in named buffers.  Params: yolo_anchor0..17 = the anchors [3][3][2] (pixels, stride 32 first), yolo_conf_thresh (0.5), yolo_nms_thresh (0.4),
 * yolo_pre_nms_top_n (1024, 1..1024), yolo_multi_label (1), yolo_min_wh (0), detections_per_img, detections_cap, nms_ge / nms_plus_one (0 here) /
 * nms_index_order.  fp32 only: "fp16" and "graph" are refused by name. */
int isegmi_yolov3_forward(isegmi_engine* e, const float* d_images_nhwc3, int N);
/* ViT classifier (model_kind 7; [UPSTREAM-RECALL] Dosovitskiy et al. in the timm layout, unverified): d_images NHWC3 fp32 [N][H][W][3],
 * normalised.  patchify -> patch_embed.proj (1x1 over P * P * 3, + position embedding) -> depth pre-LN blocks (LayerNorm, qkv, isegmi_op_attention,
 * proj + x, LayerNorm, fc1, GELU, fc2 + x) -> LayerNorm of the class tokens -> head -> isegmi_op_class_softmax -> isegmi_op_topk.  Layers by set_conv
 * (bias as shift): patch_embed.proj, blocks.<i>.attn.qkv / .attn.proj / .mlp.fc1 / .mlp.fc2, head; tensors by set_tensor: blocks.<i>.norm1 / .norm2 and
 * norm (.weight, .bias), vit.cls_row [D] = cls_token + pos_embed[0], vit.pos_rows [max_batch][T - 1][D] = pos_embed[1:] tiled.  Params: vit_dim,
 * vit_depth, vit_heads (vit_dim = 64 vit_heads), vit_mlp_dim, vit_patch (16 or 32), vit_num_classes (2..8192), vit_ln_eps (1e-6), vit_gelu_tanh (0),
 * vit_topk (5, 1..64).  Results: cls.logits / cls.prob [N][classes], cls.topk_val (probabilities) / cls.topk_idx [N][k]; vit.tokens, vit.qkv, vit.attn,
 * vit.mlp hold the embedding and the last block's tensors.  fp32 only: "fp16" and "graph" are refused by name. */
int isegmi_vit_forward(isegmi_engine* e, const float* d_images_nhwc3, int N);
/* Masker paste of the last forward into (out_h,out_w) planes; boxes first scaled by h_ratios_wh [N][2] =
 * (out_w/w_i, out_h/h_i) like BoxList.resize -> det.masks u8 [N][cap][out_h][out_w], det.box_resized */
int isegmi_maskrcnn_paste(isegmi_engine* e, const float* h_ratios_wh, int out_h, int out_w);
/* Pose2Seg test.py's model([img], [kpts]) (kind 3): d_u8_staging = the N images' [h][w][3] uint8 pixels back to back
 * (h_sizes_hw [N][2]), d_kpts = their persons' COCO keypoints [R][17][3] fp32, image by image (h_counts [N], each <= param "max_instances",
 * default 32, else ISEGMI_ERR_ARG); both may be the destinations of isegmi_engine_upload_async.  Letterbox, ResNet-FPN to P2, template fit,
 * Affine-Align, skeleton features, SegModule, then det.masks u8 [N][K][Hmax][Wmax] (each image at its own size), det.box_resized (tight xyxy,
 * right / bottom exclusive), det.score = 1, det.label = 1, det.count: isegmi_engine_rle and isegmi_engine_pack_coco_records work as for
 * Mask R-CNN.  Intermediates: p2s.p2, p2s.roi, p2s.logits, p2s.fit.  Params: cat_skeleton, align_corners, warp_round_u8, swap_rb,
 * fpn_bilinear; fp16 and graph are refused (ISEGMI_ERR_ARG). */
int isegmi_pose2seg_forward(isegmi_engine* e, const uint8_t* d_u8_staging, const int32_t* h_sizes_hw, const float* d_kpts,
                            const int32_t* h_counts, int N);
/* The same forward in its two halves, for persons that are produced on the device while the backbone already runs:
 *   body:    everything that does not depend on the persons -- per-image table, letterbox, ResNet body, FPN down to p2s.p2 -- of the N images;
 *   persons: template fit ... masks of the body's batch.  d_kpts [R][17][3] device memory, h_counts [N] on the host (they size the activations).
 *            producer_stream != NULL: d_kpts (and d_scores) were written by work enqueued on that stream so far; the main stream waits for an event
 *            recorded there instead of for an upload.  d_scores != NULL: [N][max_instances] fp32, det.score takes them in the live slots (k < h_counts[n])
 *            in place of 1; every other slot and buffer is as isegmi_pose2seg_forward leaves it.
 * isegmi_pose2seg_forward is body then persons(d_kpts, NULL, h_counts, NULL).  persons without a body of this engine in front is ISEGMI_ERR_STATE.
 *   wait_persons: host wait until the last persons call that took d_kpts from a producer stream has finished reading it and its d_scores -- and with it
 *            that step's body and image upload: the WAR point for the producer's next write into d_kpts and for the caller's pinned image buffer, and a
 *            producer loop's bound on the steps it keeps in flight (two sets of buffers: two steps). */
int isegmi_pose2seg_body(isegmi_engine* e, const uint8_t* d_u8_staging, const int32_t* h_sizes_hw, int N);
int isegmi_pose2seg_persons(isegmi_engine* e, const float* d_kpts, const float* d_scores, const int32_t* h_counts, void* producer_stream);
int isegmi_pose2seg_wait_persons(isegmi_engine* e, const float* d_kpts);
/* isegmi_op_pose_handoff on the results stream of a Keypoint R-CNN engine (model_kind 2, "keypoint_on" 1), from the det.score / det.count / det.kpt /
 * det.kscore buffers of its last forward; h_ratios_wh [N][2] on the host as for isegmi_engine_pack_keypoint_records, K = the Pose2Seg engine's
 * max_instances; the four outputs are the caller's device buffers (N * K rows of keypoints).  An engine without keypoint_on and a call before the first
 * forward are refused by name.  The caller downloads d_count_out (isegmi_engine_download_async / _wait of THIS engine) to size the Pose2Seg step. */
int isegmi_engine_pose_handoff(isegmi_engine* kp_engine, const float* h_ratios_wh, float person_thresh, float kp_thresh, int K, float* d_kpts_out,
                               float* d_score_out, int32_t* d_src_slot, int32_t* d_count_out);
/* postprocess (Y7): masks of the last forward at (out_h,out_w) -> det.masks u8, det.box_int i64 */
int isegmi_yolact_postprocess(isegmi_engine* e, int out_h, int out_w);
/* the same with image n assembled at ITS (h, w) = h_image_hw[n] inside a common plane of the batch's maximum size (a batch of images of
 * different original sizes; upstream's evalimage postprocesses one image at a time at its own size) */
int isegmi_yolact_postprocess_sizes(isegmi_engine* e, const int32_t* h_image_hw, int N);
int isegmi_engine_sync(isegmi_engine* e);
int isegmi_engine_stream(isegmi_engine* e, void** stream);
/* asynchronous H2D of an input batch from PINNED host memory on the engine's copy stream: ordered after the previous
 * forward consumed its input, and the next forward is ordered behind it (stands where the reference's
 * jt.array(image) host->device transfer sits, README.md:311/331) */
int isegmi_engine_upload_async(isegmi_engine* e, void* d_dst, const void* h_src_pinned, int64_t bytes);
/* isegmi_op_preprocess_u8 on the engine's main stream: behind any upload_async of the bytes, in front of the next forward */
int isegmi_engine_preprocess_u8(isegmi_engine* e, const uint8_t* d_u8, int N, int Hin, int Win, float* d_out, int Hout, int Wout,
                                int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb);
/* isegmi_op_preprocess_u8_flip the same way */
int isegmi_engine_preprocess_u8_flip(isegmi_engine* e, const uint8_t* d_u8, int N, int Hin, int Win, float* d_out, int Hout, int Wout,
                                     int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, int hflip);
/* isegmi_op_resample_u8 (fp32 output) scheduled like isegmi_engine_preprocess_u8.  The image table, the coefficient tables and the original bytes
 * sit in ONE device blob (one upload): the table at byte table_off, the coefficients at coeff_off (both multiples of 4), the pixels from src_off.
 * When the blob is the destination of a pending upload_async the launch goes to the copy stream behind it, otherwise to the main stream. */
int isegmi_engine_resample_u8(isegmi_engine* e, const uint8_t* d_blob, int64_t blob_bytes, int64_t table_off, const int32_t* h_table, int N,
                              int64_t coeff_off, int64_t coeff_words, int64_t src_off, float* d_out, int planes, int Hpad, int Wpad,
                              int64_t out_img_stride, const float* mean3, const float* std3, int swap_rb, float fill);
/* per-step completion marks on the results stream; step_times returns the intervals between consecutive marks (ms) */
int isegmi_engine_mark_step(isegmi_engine* e);
int isegmi_engine_step_times(isegmi_engine* e, float* ms, int cap, int* count);
/* host wait for the mark `back` marks before the newest (0 = newest): a producer loop's bound on the steps it keeps in flight */
int isegmi_engine_wait_mark(isegmi_engine* e, int back);
/* dtype: 0 f32, 1 i32, 2 u8, 3 i64; shape4 receives up to 4 dims */
int isegmi_engine_buffer_info(isegmi_engine* e, const char* name, void** d_ptr, int64_t* bytes,
                              int32_t* dtype, int64_t* shape4, int32_t* ndim);
/* device memory held by the engine: packed weights + constant tensors, and activation / workspace / output buffers (bytes) */
int isegmi_engine_memory(isegmi_engine* e, int64_t* weight_bytes, int64_t* buffer_bytes);
/* Diagnostic: which of the engine's ten streams (0 main, 1-3 side, 4 tail, 5 heads, 6-8 heads-side, 9 copy) share an in-order hardware queue of the
 * runtime (equal class numbers = one queue; found by a spin-kernel probe, ~2 ms; call on an idle engine).  An engine's throughput depends on this
 * placement, which the runtime derives from the process's stream-creation history. */
int isegmi_engine_stream_layout(isegmi_engine* e, int32_t* queue_class, int n);
/* Backbone lanes of the Yolact fp32 engine (parameter "step_overlap": consecutive forwards alternate between two lanes -- a main stream with its side
 * streams and its own backbone / FPN buffers -- so that step i + 1's backbone overlaps step i's; 0 = one lane, launch for launch as before).  n >= 18:
 * out[0] lanes the next forward alternates over (2, or 1: off, forced off -- graph capture / "graph", multi_stream 0, fp16, timing modes, other models --
 * or fallback); out[1] = 1: wanted, but the runtime gave lane 1's main stream no hardware queue apart from lane 0's main and the tail: the engine fell
 * back to one lane; out[2..11] the ten roles' queue classes as isegmi_engine_stream_layout; out[12..15] lane 1's main / side0-2 in the same numbering
 * (-1 not dealt); out[16] lanes the last forward alternated over; out[17] forwards run on lane 1 so far.  Call on an idle engine. */
int isegmi_engine_lane_layout(isegmi_engine* e, int32_t* out, int n);
/* per-stage hipEvent timings of the last synchronised forward (set_param "timing" 1 first) */
int isegmi_engine_get_timings(isegmi_engine* e, char* names, int names_cap, float* ms, int ms_cap,
                              int* count);

/* ---- device-side COCO output (README.md:344-347, 243-249): what inference() / eval ship per batch ----
 * isegmi_engine_rle: isegmi_op_rle_encode over det.masks of the last postprocess / paste on the results stream; h_image_hw [N][2] = every
 *   image's own (h, w) inside the mask planes (NULL: the whole plane) -> buffers rle.run_off / rle.counts / rle.str_off / rle.chars /
 *   rle.status.  Capacities: params "rle_cap_runs" / "rle_cap_chars" (default 256 Ki entries / bytes per image of max_batch).
 * isegmi_engine_pack_coco_records: ONE block of fixed size for n_block image slots (>= the last forward's batch: a short last batch still
 *   fills a block of the per-step size; the extra slots carry count 0) (layout: csrc/results.cpp, mirrored by isegmi/dist.py):
 *   status, boxes in original-image coordinates, counts, scores, labels, [mask scores], string offsets, RLE strings.
 * isegmi_engine_download_*: the block's asynchronous D2H into pinned memory on the results stream, behind its producer (two slots). */
int isegmi_engine_rle(isegmi_engine* e, const int32_t* h_image_hw);
int isegmi_engine_coco_record_bytes(isegmi_engine* e, int N, int64_t* bytes, int64_t* chars_offset);
int isegmi_engine_pack_coco_records(isegmi_engine* e, void* d_dst, int64_t cap, int n_block, int64_t* bytes);
/* Box-only record block of the last forward of a Mask R-CNN-family engine (Faster R-CNN: set_param "mask_on" 0), ONE launch on the results stream:
 *   [status i32 x 4 = 0][box f32 x n_block*K*4][count i32 x n_block][score f32 x n_block*K][label i32 x n_block*K], every section starting on a multiple
 *   of 8 bytes; box = det.box * (ratio_w, ratio_h, ratio_w, ratio_h) in fp32 -- xyxy in ORIGINAL image coordinates, h_ratios_wh [N][2] as for
 *   isegmi_maskrcnn_paste.  No string offsets, no characters; image slots past the last forward's batch are zero.
 * isegmi_engine_coco_record_bytes returns this block's size (chars_offset = the size) while the engine's "mask_on" is 0. */
int isegmi_engine_pack_box_records(isegmi_engine* e, const float* h_ratios_wh, void* d_dst, int64_t cap, int n_block, int64_t* bytes);
/* Keypoint record block of the last forward of a Keypoint R-CNN engine (set_param "keypoint_on" 1), ONE launch on the results stream: the
 *   box-only block above with two more sections behind label, [kpt f32 x n_block*K*NK*3][kscore f32 x n_block*K*NK] (NK keypoints per detection): kpt's x and
 *   y = det.kpt * (ratio_w, ratio_h), one fp32 multiplication each, v copied; every section starts on a multiple of 8 bytes, unused slots are zero.
 * isegmi_engine_coco_record_bytes returns this block's size (chars_offset = the size) while the engine's "keypoint_on" is 1. */
int isegmi_engine_pack_keypoint_records(isegmi_engine* e, const float* h_ratios_wh, void* d_dst, int64_t cap, int n_block, int64_t* bytes);
/* isegmi_op_paint over the engine's det.masks rows of image `image_index` of the last paste / postprocess, on the stream that produced them and ordered
 * behind it; the lists are HOST arrays (checked, then staged by the engine), d_image / d_out the caller's device buffers.  ISEGMI_ERR_STATE by name: a call
 * before the first forward; an entry that names a slot while there is no det.masks of this batch (no paste / postprocess yet, a box-only engine, RetinaNet,
 * YOLOv3: those paint with slot -1 only) or while "sparse_masks" leaves the planes incomplete. */
int isegmi_engine_paint(isegmi_engine* e, int image_index, const uint8_t* d_image, int H, int W, const int32_t* h_entries, int D, const int32_t* h_dots,
                        int Q, uint8_t* d_out);
int isegmi_engine_download_async(isegmi_engine* e, int slot, void* h_dst_pinned, const void* d_src, int64_t bytes);
int isegmi_engine_download_fence(isegmi_engine* e, int slot);
int isegmi_engine_download_wait(isegmi_engine* e, int slot);

/* one contiguous record block of the last Yolact forward for the all-gather:
 * [count i32 N][box f32 N*K*4][score f32 N*K][class i32 N*K][coeff f32 N*K*32]([proto f32 N*PH*PW*32]) */
int isegmi_yolact_pack_records(isegmi_engine* e, void* d_dst, int64_t cap, int with_proto, int64_t* bytes);

/* Mask R-CNN record block for the all-gather:
 * [count i32 N][box f32 N*K*4][score f32 N*K][label i32 N*K][mask28 f32 N*K*784] */
int isegmi_maskrcnn_pack_records(isegmi_engine* e, void* d_dst, int64_t cap, int64_t* bytes);

/* conv-kernel statistics since the last call (set_param "conv_timing" 1): algorithmic FLOPs, summed
 * HIP-event time (ms) of the conv launches on the engine stream, launch count; resets them */
int isegmi_engine_conv_stats(isegmi_engine* e, double* flops, double* ms, int64_t* launches);
/* HBM-bound (non-conv) stages under set_param("op_timing", 1): per stage label the summed HIP-event time (us, on the stream the stage is
 * launched on), its ALGORITHMIC bytes and the number of timed scopes since the last call; labels joined by '\n' in `names`.
 * Call after isegmi_engine_sync.  Resets the accumulators.  (bench.py: roofline_hbm) */
int isegmi_engine_op_stats(isegmi_engine* e, char* names, int names_cap, double* us, double* bytes, int64_t* launches, int cap, int* count);

/* per-layer text report (label, GFLOP, ms, TFLOP/s per line) accumulated under conv_timing; clears it */
int isegmi_engine_conv_report(isegmi_engine* e, char* buf, int cap);

/* ---- COCO evaluation on the device (csrc/cocoeval.hip) ----
 * What of pycocotools' maskApi.c / cocoeval.py these restate (rleArea, rleToBbox, rleIou, bbIou, COCOeval.computeOks / evaluateImg) is
 * [UPSTREAM-RECALL -- unverified].  An RLE is its run counts as isegmi.coco.rle_from_string yields them: column-major, zeros first.
 * M RLEs lie back to back in d_counts; d_off [M + 1] (int64) are their first runs; d_hw [M][2] = (h, w), h * w < 2^32.
 *
 * isegmi_op_rle_prefix: d_bounds[i] = end position of run i, d_cum[i] = set pixels in runs 0 .. i (both per RLE, same indexing as d_counts);
 *   d_area [M] = set pixels; d_bbox [M][4] = tight box (x0, y0, x1, y1) INCLUSIVE, (0, 0, -1, -1) for an empty mask.
 * isegmi_op_rle_iou: d_pairs [P][3] = (det RLE, gt RLE, crowd); d_out[p] = inter / union, inter / area(det) when crowd, exactly 0.0 when
 *   inter == 0.  inter and the areas are integers; the only floating operation is one double division.  -1.0 marks a pair that is not
 *   evaluable (an index outside [0, M), or two RLEs of different size).
 * isegmi_op_bbox_iou: the same pair list over d_boxes [B][4] double xywh, in bbIou's operation order:
 *   da = dw*dh; ga = gw*gh; w = min(dx+dw, gx+gw) - max(dx, gx), w <= 0 -> 0; h likewise; i = w*h; u = crowd ? da : (da + ga) - i; o = i / u. */
int isegmi_coco_rle_prefix_bytes(int64_t total_runs, int M, int64_t* bounds_bytes, int64_t* cum_bytes, int64_t* area_bytes, int64_t* bbox_bytes);
int isegmi_op_rle_prefix(const uint32_t* d_counts, const int64_t* d_off, const int32_t* d_hw, int M, uint32_t* d_bounds, uint32_t* d_cum,
                         int64_t* d_area, int32_t* d_bbox, void* stream);
int isegmi_op_rle_iou(const uint32_t* d_bounds, const uint32_t* d_cum, const int64_t* d_off, const int32_t* d_hw, const int64_t* d_area,
                      const int32_t* d_bbox, int M, const int32_t* d_pairs, int64_t P, double* d_out, void* stream);
int isegmi_op_bbox_iou(const double* d_boxes, int B, const int32_t* d_pairs, int64_t P, double* d_out, void* stream);
/* isegmi_op_oks: object keypoint similarity of the same pair list ([UPSTREAM-RECALL -- unverified] COCOeval.computeOks).  M items (gts and
 * dets in one list): d_kpts [M][K][3] = (x, y, v), d_box [M][4] xywh and d_area [M] (read for a gt only), d_vars [K] = (sigmas * 2) ** 2 as the
 * host computes it, 1 <= K <= 32; d_pairs [P][3] = (det item, gt item, unused).  Per pair, every operation one IEEE double operation in this order:
 *   k1 = #{k : vg_k > 0}
 *   k1 > 0 : only the keypoints with vg_k > 0 count;  dx = xd - xg, dy = yd - yg
 *   k1 == 0: all K count;  x0 = bx - bw, x1 = bx + bw*2, dx = max(0, x0 - xd) + max(0, xd - x1), y likewise
 *   e = ((dx*dx + dy*dy) / vars_k) / (area + 2^-52) / 2;   d_out[p] = (sum of exp(-e)) / n,  n = k1, or K when k1 == 0
 * The terms are added in keypoint-index order by one add each (upstream's np.sum uses another order: a deliberate deviation).  A keypoint
 * that does not count is selected out, so its coordinates may be anything, NaN included; the detection's v is never read.  A pair's value
 * depends on its two items alone, not on P or on the other pairs.  -1.0 marks an item index outside [0, M). */
int isegmi_op_oks(const double* d_kpts, const double* d_box, const double* d_area, const double* d_vars, int M, int K, const int32_t* d_pairs,
                  int64_t P, double* d_out, void* stream);
/* isegmi_op_coco_match: evaluateImg's greedy matching, one sequential scan per (group, area range, IoU threshold).  A group is one
 * (image, category) -- or one image with useCats = 0.  Group g owns detections [d_det_off[g], d_det_off[g + 1]) (already sorted by score, best
 * first, and cut to maxDets[-1]), gts [d_gt_off[g], d_gt_off[g + 1]) and the row-major [D][G] IoU block at d_ious + d_iou_off[g].
 * Rule per area range a = (lo, hi) and threshold t: gtIg = ignore | iscrowd | area < lo | area > hi; gts are visited non-ignored first, each
 * part in input order; every det in turn starts with best = min(t, 1 - 1e-10), skips a gt matched at this t unless it is crowd, stops at the
 * first ignored gt once it holds a non-ignored match, skips iou < best, else takes the gt and raises best.  A matched det inherits the gt's
 * ignore flag; an unmatched det whose own area lies outside a is ignored.
 * Outputs (sizes: isegmi_coco_match_bytes): d_dt_match [A][T][n_dets] = 1 + the gt's index inside its group (input order), 0 = unmatched
 * (upstream stores the annotation id, so that a gt with id 0 looks unmatched: a deliberate deviation); d_dt_ignore [A][T][n_dets];
 * d_gt_match [A][T][n_gts] = 1 + the det's index inside its group, 0 = unmatched; d_gt_ignore_out [A][n_gts]. */
typedef struct isegmi_coco_match_args {
    int32_t n_groups, A, T, reserved;
    int64_t n_dets, n_gts, n_ious;
    const int64_t* d_det_off;      /* [n_groups + 1] */
    const int64_t* d_gt_off;       /* [n_groups + 1] */
    const int64_t* d_iou_off;      /* [n_groups] */
    const double* d_ious;          /* [n_ious] */
    const double* d_det_area;      /* [n_dets] */
    const double* d_gt_area;       /* [n_gts] */
    const uint8_t* d_gt_crowd;     /* [n_gts] */
    const uint8_t* d_gt_ignore;    /* [n_gts] */
    const double* d_area_rng;      /* [A][2] */
    const double* d_iou_thrs;      /* [T] */
    int32_t* d_dt_match;
    uint8_t* d_dt_ignore;
    int32_t* d_gt_match;
    uint8_t* d_gt_ignore_out;
} isegmi_coco_match_args;
int isegmi_coco_match_bytes(int64_t n_dets, int64_t n_gts, int A, int T, int64_t* dt_match_bytes, int64_t* dt_ignore_bytes,
                            int64_t* gt_match_bytes, int64_t* gt_ignore_bytes);
int isegmi_op_coco_match(const isegmi_coco_match_args* a, void* stream);

/* ---- multi-GPU: images shard by batch, one process per GPU; the only exchange is one
 * RCCL all-gather of fixed-size records per batch (upstream analogue: the pickle all_gather of
 * {image_id: BoxList} in maskrcnn-benchmark engine/inference.py, reached from README.md:344-347). */
typedef struct isegmi_comm isegmi_comm;
int isegmi_comm_unique_id(void* out128);                       /* rank 0; ship the 128 bytes to all ranks */
int isegmi_comm_create(const void* uid128, int rank, int world, isegmi_comm** out);
int isegmi_comm_destroy(isegmi_comm* c);
/* d_recv holds world*bytes; runs on producer_stream behind the work already queued there (NULL: the communicator's own stream) */
int isegmi_comm_allgather(isegmi_comm* c, const void* d_send, void* d_recv, int64_t bytes,
                          void* producer_stream);
int isegmi_comm_wait(isegmi_comm* c);
/* Two record slots (0, 1) so that step t+1 packs while step t gathers, without a host sync in between:
 *   fence_producer(slot, s): work enqueued on stream s afterwards runs after the slot's last all-gather finished (WAR);
 *   allgather_slot: as isegmi_comm_allgather (= slot 0) through the given slot; wait_slot: host wait for that slot. */
int isegmi_comm_fence_producer(isegmi_comm* c, int slot, void* producer_stream);
int isegmi_comm_allgather_slot(isegmi_comm* c, int slot, const void* d_send, void* d_recv, int64_t bytes,
                               void* producer_stream);
int isegmi_comm_wait_slot(isegmi_comm* c, int slot);
/* Collectives of one communicator run in the order the host issued them, whatever streams they were given: one that goes to another stream than its
 * predecessor first makes that stream wait for the predecessor's completion event.  out4 = {rank, world, collectives issued, how many of them changed
 * stream} (diagnostic: isegmi.dist keeps every data step, empty step and redo of a run on ONE stream, so the last number stays 0 between control words). */
int isegmi_comm_info(isegmi_comm* c, int64_t* out4);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
