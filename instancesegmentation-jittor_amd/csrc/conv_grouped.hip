// conv_grouped.hip -- grouped 3x3 convolution (ResNeXt conv2) on v_mfma_f32_16x16x4_f32 (gfx950), fp32 NHWC.
//
// Numerics contract: the fp32 one of conv_mfma.hip / ora_conv2d, applied per group.  Output channel co of group g = co / cg (cg = C / groups) is ONE chain
// acc = fmaf(x_k, w_k, acc) from +0 over k = (r, s, c) ascending, c running over the group's OWN cg input channels; padding taps are x = 0 products; then
// y = fmaf(acc, scale, shift) + residual -> activation.  cg <= 64 < 128, so the 128-channel K-group rule of conv_korder.h never applies.  The 16x16x4 MFMA
// is bit for bit such a chain, 4 k deep (see the 16x16x4 kernels of conv_mfma.hip).  No output ever meets an input channel of another group: there is no
// dense GEMM over zero-padded weights, so a non-finite activation stays inside its group (inf * 0 = NaN would leak it).
//
// The layer is memory-bound (1/32 of the dense FLOPs on the same activations), so the kernel is built around touching HBM once:
//   * a block owns TH output rows x 16 output columns of one image x a 64-channel slab (64 / cg whole groups) and stages the input window with its halo,
//     those 64 channels only, in LDS once (TH = 8 or 4 at stride 1, 2 at stride 2: conv2d_grouped_launch; pixel pitch 66 floats: the 16 pixels x 2 k of a ds_read_b32 half land on 32 different banks at stride 1);
//   * wave t of the four owns the slab's 16 output channels 16 t .. 16 t + 15 for EVERY pixel row of the block: its weights are its own (no wave loads
//     another's), come from a packed image in which one (tap, k-step) fragment is 64 consecutive floats in lane order (one coalesced load per wave),
//     and are prefetched a tap ahead;
//   * the MFMA runs transposed (A = weights, rows = output channels; B = pixels, columns = output pixels), so a lane ends up with FOUR CONSECUTIVE output
//     channels of one pixel: residual loads and output stores are 16-byte accesses, skipped for pixels past the image;
//   * cg = 8: a 16-channel tile holds two groups.  Each gets its own accumulator and its own MFMA fed with its own 8 input channels (the other group's eight
//     rows of that MFMA are dummies); a lane select (rows 0-7 / 8-15 = lane quads 0-1 / 2-3) merges them.  Half the MFMA issue of res2 is wasted; res2 is
//     the most memory-bound of the four stages.
#include "../../include/isegmi.h"
#include "common.h"

namespace isegmi {

typedef float gf32x4 __attribute__((ext_vector_type(4)));

struct GConvK {
    const float* in;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* out;
    int N, H, W, C, Ho, Wo;
    int tiles_x, tiles_y, slabs;
    int act;
};

constexpr int GC_PITCH = 66;   // floats per staged pixel: 64 channels + 2 (bank = 2 * pixel + k for the fragment reads)

template <int CG, int STRIDE, int TH>
__global__ __launch_bounds__(256) void conv_grouped_kernel(const GConvK p) {
    constexpr int WROWS = (TH - 1) * STRIDE + 3, WCOLS = 15 * STRIDE + 3;
    constexpr int STEPS = CG / 4;          // MFMAs (4 k each) per tap and group
    constexpr int NA = CG == 8 ? 2 : 1;    // accumulators per pixel row: one per group inside the wave's 16 channels
    constexpr int NV = WROWS * WCOLS * 16; // float4s of the window
    constexpr int NL = (NV + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) float gsm[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // XCD-aware bijective remap (as conv_mfma.hip): an XCD takes a contiguous range of the walk (slab fastest, then columns, rows, images), so that the
    // halo a tile shares with its neighbours is served by that XCD's L2
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int slab = logical % p.slabs; logical /= p.slabs;
    const int tx = logical % p.tiles_x; logical /= p.tiles_x;
    const int ty = logical % p.tiles_y;
    const int n = logical / p.tiles_y;

    // ---- stage the window: pixel (wy, wx) of the window is input pixel (h0 + wy, w0 + wx), zero outside the image.  Every load goes to an address inside
    // the image (coordinates clamped; the value is dropped by a select): no branch around a load, all of a thread's loads in flight together.
    const int h0 = ty * TH * STRIDE - 1, w0 = tx * 16 * STRIDE - 1;
    const float* const src = p.in + (size_t)n * p.H * p.W * p.C + slab * 64;
    float4 v[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int idx = tid + 256 * j;
        const int pix = idx >> 4, c4 = idx & 15;
        const int wy = pix / WCOLS, wx = pix - wy * WCOLS;
        const int hi = h0 + wy, wi = w0 + wx;
        const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        const int hc = min(max(hi, 0), p.H - 1), wc = min(max(wi, 0), p.W - 1);
        const float4 t = *(const float4*)(src + (size_t)(hc * p.W + wc) * p.C + c4 * 4);
        v[j] = ok ? t : float4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int idx = tid + 256 * j;
        if (idx < NV) {
            float* d = gsm + (idx >> 4) * GC_PITCH + (idx & 15) * 4;   // 8-byte aligned at this pitch
            *(float2*)d = float2{v[j].x, v[j].y};
            *(float2*)(d + 2) = float2{v[j].z, v[j].w};
        }
    }
    __syncthreads();

    // ---- MFMA loop.  Lane (i = lane & 15, q = lane >> 4) supplies k = 4 step + q: A = weight of output channel 16 wave + i, B = pixel column i.
    const int li = lane & 15, lq = lane >> 4;
    const float* wp = p.w + (size_t)(slab * 4 + wave) * (9 * STEPS * 64) + lane;
    const int cb0 = CG == 8 ? wave * 16 : (wave * 16 / CG) * CG;   // first slab channel of the (first) group of the wave's 16 output channels
    const float* lb = gsm + li * STRIDE * GC_PITCH + cb0 + lq;

    gf32x4 acc[NA][TH];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int m = 0; m < TH; ++m) acc[a][m] = gf32x4{0.0f, 0.0f, 0.0f, 0.0f};

    float wf[STEPS], wn[STEPS];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) wf[st] = wp[st * 64];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int nt = tap < 8 ? tap + 1 : 8;   // the next tap's weights travel under this tap's MFMAs
#pragma unroll
        for (int st = 0; st < STEPS; ++st) wn[st] = wp[(nt * STEPS + st) * 64];
        const int r = tap / 3, s = tap - 3 * r;
        const float* lt = lb + (r * WCOLS + s) * GC_PITCH;
#pragma unroll
        for (int st = 0; st < STEPS; ++st)
#pragma unroll
            for (int m = 0; m < TH; ++m)
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const float x = lt[m * STRIDE * WCOLS * GC_PITCH + a * 8 + 4 * st];
                    acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[st], x, acc[a][m], 0, 0, 0);
                }
#pragma unroll
        for (int st = 0; st < STEPS; ++st) wf[st] = wn[st];
    }

    // ---- epilogue.  D: row (output channel of the tile) = 4 q + e, column (pixel) = i.  y = fmaf(acc, scale, shift) + residual -> act, as epi_finish.
    const int co = slab * 64 + wave * 16 + 4 * lq;
    float sc[4], sh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sc[e] = p.scale ? p.scale[co + e] : 1.0f;
        sh[e] = p.shift ? p.shift[co + e] : 0.0f;
    }
    const int xo = tx * 16 + li;
#pragma unroll
    for (int m = 0; m < TH; ++m) {
        const int yo = ty * TH + m;
        if (xo < p.Wo && yo < p.Ho) {
            const size_t off = ((size_t)(n * p.Ho + yo) * p.Wo + xo) * p.C + co;
            gf32x4 a = acc[0][m];
            if (CG == 8) a = lq < 2 ? acc[0][m] : acc[NA - 1][m];
            const float4 rv = p.res ? *(const float4*)(p.res + off) : float4{0.0f, 0.0f, 0.0f, 0.0f};
            const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = fmaf(a[e], sc[e], sh[e]) + rr[e];   // + (+0) without a residual, as epi_finish
                if (p.act == 1) y[e] = y[e] > 0.0f ? y[e] : 0.0f;
            }
            *(float4*)(p.out + off) = float4{y[0], y[1], y[2], y[3]};
        }
    }
}

// The supported set (include/isegmi.h): 3x3 / pad 1 / stride 1 or 2, Cin == Cout a multiple of 64, cg = Cin / groups in {8, 16, 32, 64}, act 0 or 1, dense output.
static int check_grouped(const isegmi_conv_desc* d, int groups) {
    ARG_CHECK(d != nullptr, "null desc");
    ARG_CHECK(d->N >= 0 && d->H >= 0 && d->W >= 0, "negative conv geometry");
    ARG_CHECK(d->R == 3 && d->S == 3 && d->pad == 1, "grouped conv: R = S = 3, pad = 1 only");
    ARG_CHECK(d->stride == 1 || d->stride == 2, "grouped conv: stride 1 or 2 only");
    ARG_CHECK(d->Cin > 0 && d->Cin == d->Cout && d->Cin % 64 == 0, "grouped conv: Cin == Cout, a multiple of 64");
    ARG_CHECK(groups >= 1 && d->Cin % groups == 0, "grouped conv: groups must divide Cin");
    const int cg = d->Cin / groups;
    ARG_CHECK(cg == 8 || cg == 16 || cg == 32 || cg == 64, "grouped conv: Cin / groups must be 8, 16, 32 or 64");
    ARG_CHECK(d->act == 0 || d->act == 1, "grouped conv: act 0 or 1");
    ARG_CHECK(d->tile == 0, "grouped conv: tile must be 0");
    ARG_CHECK(d->out_div == 0 && d->out_img_stride == 0 && d->out_pix_stride == 0, "grouped conv: dense contiguous output only");
    return ISEGMI_OK;
}

template <int CG, int STRIDE, int TH>
static int grouped_launch_as(GConvK& k, hipStream_t st) {
    constexpr int WROWS = (TH - 1) * STRIDE + 3, WCOLS = 15 * STRIDE + 3;
    const size_t lds = (size_t)WROWS * WCOLS * GC_PITCH * sizeof(float);
    k.tiles_y = cdiv(k.Ho, TH);
    k.tiles_x = cdiv(k.Wo, 16);
    const int64_t blocks = (int64_t)k.N * k.tiles_y * k.tiles_x * k.slabs;
    ARG_CHECK(blocks < (1ll << 31), "grouped conv: too many tiles");
    LDS_LIMIT_ONCE((int)lds, conv_grouped_kernel<CG, STRIDE, TH>);
    hipLaunchKernelGGL((conv_grouped_kernel<CG, STRIDE, TH>), dim3((unsigned)blocks), dim3(256), lds, st, k);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int conv2d_grouped_launch(const isegmi_conv_desc* d, int groups, const float* in, const float* w, const float* scale, const float* shift, const float* res,
                          float* out, hipStream_t st) {
    const int rc = check_grouped(d, groups);
    if (rc) return rc;
    GConvK k;
    k.N = d->N; k.H = d->H; k.W = d->W; k.C = d->Cin;
    k.Ho = (d->H - 1) / d->stride + 1;
    k.Wo = (d->W - 1) / d->stride + 1;
    if (d->N == 0 || d->H == 0 || d->W == 0) return ISEGMI_OK;   // M == 0: nothing to do
    ARG_CHECK(in && w && out, "null device pointer");
    ARG_CHECK((int64_t)d->N * d->H * d->W * d->Cin < (1ll << 31), "grouped conv: input must be < 2^31 elements");
    k.in = in; k.w = w; k.scale = scale; k.shift = shift; k.res = res; k.out = out;
    k.slabs = d->Cin / 64;
    k.act = d->act;
    const int cg = d->Cin / groups;
    // Rows per block, measured per shape (tools/grouped_conv_bench.py).  Stride 1: 8 rows (10 x 18 window, 47.5 KB, three blocks per CU) for
    // cg = 8, whose two MFMAs per fragment keep the CU busy, and for cg = 64, whose 147 KB of weights per block want the reuse; 4 rows (6 x 18, 28.5 KB, five
    // blocks per CU: more blocks to cover each other's staging phase) for cg = 16 and 32, 9-15 % faster there.  Stride 2: 2 rows (5 x 33, 43.6 KB, three blocks
    // per CU), 7-14 % ahead of 4 rows.
    if (d->stride == 1) {
        switch (cg) {
            case 8: return grouped_launch_as<8, 1, 8>(k, st);
            case 16: return grouped_launch_as<16, 1, 4>(k, st);
            case 32: return grouped_launch_as<32, 1, 4>(k, st);
            default: return grouped_launch_as<64, 1, 8>(k, st);
        }
    }
    switch (cg) {
        case 8: return grouped_launch_as<8, 2, 2>(k, st);
        case 16: return grouped_launch_as<16, 2, 2>(k, st);
        case 32: return grouped_launch_as<32, 2, 2>(k, st);
        default: return grouped_launch_as<64, 2, 2>(k, st);
    }
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_conv_grouped_packed_floats(const isegmi_conv_desc* d, int groups, int64_t* n) {
    const int rc = check_grouped(d, groups);
    if (rc) return rc;
    ARG_CHECK(n != nullptr, "null pointer");
    *n = (int64_t)d->Cout * 9 * (d->Cin / groups);
    return ISEGMI_OK;
}

// packed[slab][tile t of 16 channels][tap][k-step][lane (q, i)] = w[64 slab + 16 t + i][tap][4 step + q]: a bijection of the source weights
extern "C" int isegmi_pack_conv_weights_grouped(const isegmi_conv_desc* d, int groups, const float* w, float* packed) {
    const int rc = check_grouped(d, groups);
    if (rc) return rc;
    ARG_CHECK(w && packed, "null pointer");
    const int cg = d->Cin / groups, steps = cg / 4;
    for (int co = 0; co < d->Cout; ++co) {
        const int tile = co >> 4, i = co & 15;   // tile = 4 slab + t
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < cg; ++c) {
                const int step = c >> 2, q = c & 3;
                packed[(((int64_t)tile * 9 + tap) * steps + step) * 64 + q * 16 + i] = w[((int64_t)co * 9 + tap) * cg + c];
            }
    }
    return ISEGMI_OK;
}

extern "C" int isegmi_op_conv2d_grouped(const isegmi_conv_desc* d, int groups, const float* d_in, const float* d_w, const float* d_scale, const float* d_shift,
                                        const float* d_res, float* d_out, void* stream) {
    return conv2d_grouped_launch(d, groups, d_in, d_w, d_scale, d_shift, d_res, d_out, (hipStream_t)stream);
}
