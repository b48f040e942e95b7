// deform_conv.hip -- fused 3x3 deformable convolution (DCNv1 / DCNv2 conv2 of the dcn/ R-CNN models and of the YOLACT++ backbones) on
// v_mfma_f32_16x16x4_f32 (gfx950), fp32 NHWC.  The nine taps are sampled straight into the MFMA operand tile in LDS: the column tensor
// [N][Ho][Wo][9 C] of the unfused form (deform_im2col_kernel -> a 1x1 convolution over 9 C channels) is never written.
//
// Numerics contract: bit for bit the unfused form.  A sampled value is deform_sample.h's (the one copy both forms use).  One output is ONE chain
// acc = fmaf(a_k, w_k, acc) from +0 with the taps (r, s) outermost and all C channels of a tap ascending inside -- the K order of a 1x1 over the columns
// (conv_kgroup: one K group), NOT the 128-channel K-group walk of a plain 3x3 -- then y = fmaf(acc, scale, shift) + residual -> act, as epi_finish.  The
// 16x16x4 MFMA is bit for bit such a chain, 4 k deep (conv_mfma.hip).  Weights: the isegmi_pack_conv_weights image of the 1x1 / 9 C descriptor, as is.
//
// Shape of the kernel:
//   * a block owns DC_TP = 64 consecutive output pixels (of the flat N * Ho * Wo index) and a band of 64 NT output channels.  The kernel is written for
//     any NT (a band of all of Cout would gather once), but the launcher runs NT = 1: measured at the R-CNN shapes, bands of 128 and 256
//     are 4-100 % slower -- a wide band leaves res4 / res5 with fewer blocks than the device has CUs, and the repeated gather is served by L2;
//   * the sampling record of every (pixel, tap) of the tile -- four corner pixel indices clamped into the image, four weights, the mask factor, the live
//     bits -- is computed once into LDS;
//   * one K step is one (tap, 32-channel chunk): 64 pixels x 8 float4 = two slots per thread, each with four 16-byte corner loads, all eight in flight
//     together and issued BEFORE the MFMAs of the previous step; no branch around a load (the index is clamped, the value masked).  The samples go
//     to a double-buffered LDS image (pixel pitch 34 floats: the 16 pixels x 2 k of a ds_read_b32 half land on 32 different banks); one barrier per step;
//   * wave t of the four owns the 16-channel tiles t, t + 4, ... of the band for all 64 pixels; its weight fragments come straight from the packed rows
//     (L2) and are prefetched one step ahead;
//   * the MFMA runs transposed (A = weights, B = pixels): a lane ends with four consecutive output channels of one pixel, so residual loads and output
//     stores are 16-byte accesses.
#include "../../include/isegmi.h"
#include "common.h"
#include "conv_korder.h"
#include "deform_sample.h"

namespace isegmi {

typedef float df32x4 __attribute__((ext_vector_type(4)));

constexpr int DC_TP = 64;      // output pixels per block (tests/test_deform_conv_gpu.py states it)
constexpr int DC_PITCH = 34;   // floats per pixel of the operand image: 32 channels + 2
constexpr int DC_REC = DC_TP * 9;

struct DConvK {
    const float* x;
    const float* om;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* out;
    int N, H, W, C, Ho, Wo, M, OC, stride, Cout, cout_pad, act;
};

constexpr size_t DC_LDS = (size_t)(2 * DC_TP * DC_PITCH + 10 * DC_REC) * sizeof(float);

template <int NT, bool MOD>
__global__ __launch_bounds__(256) void deform_conv_kernel(const DConvK p) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    float* const abuf = dsm;                                    // [2][DC_TP][DC_PITCH]
    float* const rw = dsm + 2 * DC_TP * DC_PITCH;               // [5][DC_REC]: w1 w2 w3 w4 m
    int* const ri = (int*)(rw + 5 * DC_REC);                    // [5][DC_REC]: four corner pixel indices (of the whole batch), live bits

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * DC_TP;
    const int band0 = blockIdx.y * (64 * NT);

    // ---- sampling records of the tile
    for (int idx = tid; idx < DC_REC; idx += 256) {
        const int pl = idx / 9, k = idx - 9 * pl;
        const int m = m0 + pl;
        DeformTap t;
        int nb = 0;
        if (m < p.M) {
            const int wo = m % p.Wo, q = m / p.Wo;
            const int ho = q % p.Ho, n = q / p.Ho;
            const float* o = p.om + (size_t)m * p.OC;
            const int i = k / 3, j = k - 3 * i;
            const float h = (float)(ho * p.stride - 1 + i) + o[2 * k];
            const float w = (float)(wo * p.stride - 1 + j) + o[2 * k + 1];
            deform_tap(h, w, p.H, p.W, MOD ? o[18 + k] : 0.0f, MOD, t);
            nb = n * p.H * p.W;
        } else {
            deform_tap(-2.0f, -2.0f, p.H, p.W, 0.0f, MOD, t);   // a pixel past the end: dead
        }
        const int hl = min(max(t.hl, 0), p.H - 1), hh = min(max(t.hl + 1, 0), p.H - 1);
        const int wl = min(max(t.wl, 0), p.W - 1), wh = min(max(t.wl + 1, 0), p.W - 1);
        rw[idx] = t.w1; rw[DC_REC + idx] = t.w2; rw[2 * DC_REC + idx] = t.w3; rw[3 * DC_REC + idx] = t.w4; rw[4 * DC_REC + idx] = t.m;
        ri[idx] = nb + hl * p.W + wl; ri[DC_REC + idx] = nb + hl * p.W + wh; ri[2 * DC_REC + idx] = nb + hh * p.W + wl;
        ri[3 * DC_REC + idx] = nb + hh * p.W + wh; ri[4 * DC_REC + idx] = (int)t.live;
    }
    __syncthreads();

    // ---- the walk: step = (tap, 32-channel chunk), taps outermost
    const int cch = p.C >> 5, steps = 9 * cch;
    const int li = lane & 15, lq = lane >> 4;
    // weight of (row co, k = 32 step + 4 t + lq) in the packed row: groups of 8 k sit as [k0 k2 k4 k6 | k1 k3 k5 k7] (conv_perm8)
    const int wlane = conv_perm8(lq);   // t even: e = lq; t odd: e = 4 + lq = conv_perm8(lq) + 2
    unsigned wrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = min(band0 + (wave + 4 * nt) * 16 + li, p.cout_pad - 1);   // rows past Cout are the image's zero padding or a repeat: never stored
        wrow[nt] = (unsigned)co * (unsigned)(9 * p.C) + (unsigned)wlane;
    }

    const int spl = tid >> 3, sc4 = tid & 7;   // gather slots: pixels spl and spl + 32 of the tile, channels 4 sc4 .. 4 sc4 + 3 of the chunk
    float4 cv[2][4];
    unsigned lv[2];
    auto gather = [&](const int tap, const int chunk) {
        const int c0 = chunk * 32 + sc4 * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int rec = (spl + 32 * j) * 9 + tap;
            lv[j] = (unsigned)ri[4 * DC_REC + rec];
#pragma unroll
            for (int c = 0; c < 4; ++c) cv[j][c] = *(const float4*)(p.x + (size_t)ri[c * DC_REC + rec] * p.C + c0);
        }
    };
    // A dead corner and a dead position are +0: the value's bits under an all-ones or all-zeros mask.  A mask, not a select: the compiler turns selects
    // of this much arithmetic into branches and sinks the loads into them, behind the MFMAs that are there to cover their latency.
    auto keep = [](const float v, const unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); };
    auto sample = [&](const int tap, float* dst) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int rec = (spl + 32 * j) * 9 + tap;
            const float w1 = rw[rec], w2 = rw[DC_REC + rec], w3 = rw[2 * DC_REC + rec], w4 = rw[3 * DC_REC + rec], mk = rw[4 * DC_REC + rec];
            const unsigned m1 = 0u - (lv[j] & 1u), m2 = 0u - ((lv[j] >> 1) & 1u), m3 = 0u - ((lv[j] >> 2) & 1u), m4 = 0u - ((lv[j] >> 3) & 1u);
            const unsigned in = 0u - ((lv[j] >> 4) & 1u);
            const float4 c1 = cv[j][0], c2 = cv[j][1], c3 = cv[j][2], c4 = cv[j][3];
            float2 a, b;
            a.x = keep(deform_mix(w1, w2, w3, w4, mk, MOD, keep(c1.x, m1), keep(c2.x, m2), keep(c3.x, m3), keep(c4.x, m4)), in);
            a.y = keep(deform_mix(w1, w2, w3, w4, mk, MOD, keep(c1.y, m1), keep(c2.y, m2), keep(c3.y, m3), keep(c4.y, m4)), in);
            b.x = keep(deform_mix(w1, w2, w3, w4, mk, MOD, keep(c1.z, m1), keep(c2.z, m2), keep(c3.z, m3), keep(c4.z, m4)), in);
            b.y = keep(deform_mix(w1, w2, w3, w4, mk, MOD, keep(c1.w, m1), keep(c2.w, m2), keep(c3.w, m3), keep(c4.w, m4)), in);
            float* d = dst + (spl + 32 * j) * DC_PITCH + sc4 * 4;   // 8-byte aligned at this pitch
            *(float2*)d = a;
            *(float2*)(d + 2) = b;
        }
    };

    float wf[NT][8], wn[NT][8];
    auto wload = [&](const int step, float (&dstw)[NT][8]) {
        const float* wp = p.w + step * 32;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int t = 0; t < 8; ++t) dstw[nt][t] = wp[wrow[nt] + 8 * (t >> 1) + 2 * (t & 1)];
    };

    df32x4 acc[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) acc[nt][pg] = df32x4{0.0f, 0.0f, 0.0f, 0.0f};

    gather(0, 0);
    wload(0, wf);
    sample(0, abuf);
    __syncthreads();

    int ntap = 0, nchunk = 0;   // (tap, chunk) of the step after the current one
#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
        const bool more = step + 1 < steps;   // past the end: a harmless repeat (loaded, never used)
        if (more && ++nchunk == cch) { nchunk = 0; ++ntap; }
        gather(ntap, nchunk);
        wload(more ? step + 1 : step, wn);
        __builtin_amdgcn_sched_barrier(0);   // the loads above are issued HERE, ahead of the MFMAs that cover them
        const float* ab = abuf + (step & 1) * (DC_TP * DC_PITCH) + li * DC_PITCH + lq;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float xb[4];
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) xb[pg] = ab[pg * 16 * DC_PITCH + 4 * t];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int pg = 0; pg < 4; ++pg) acc[nt][pg] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nt][t], xb[pg], acc[nt][pg], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) sample(ntap, abuf + ((step + 1) & 1) * (DC_TP * DC_PITCH));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int t = 0; t < 8; ++t) wf[nt][t] = wn[nt][t];
        __syncthreads();
    }

    // ---- epilogue.  D: row (output channel of the tile) = 4 lq + e, column (pixel) = li.  y = fmaf(acc, scale, shift) + residual -> act, as epi_finish.
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = band0 + (wave + 4 * nt) * 16 + 4 * lq;
        if (co >= p.Cout) continue;   // Cout % 4 == 0: all four channels or none
        float sc[4], sh[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sc[e] = p.scale ? p.scale[co + e] : 1.0f;
            sh[e] = p.shift ? p.shift[co + e] : 0.0f;
        }
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) {
            const int m = m0 + pg * 16 + li;
            if (m >= p.M) continue;
            const size_t off = (size_t)m * p.Cout + co;
            const float4 rv = p.res ? *(const float4*)(p.res + off) : float4{0.0f, 0.0f, 0.0f, 0.0f};
            const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = fmaf(acc[nt][pg][e], sc[e], sh[e]) + rr[e];   // + (+0) without a residual, as epi_finish
                if (p.act == 1) y[e] = y[e] > 0.0f ? y[e] : 0.0f;
            }
            *(float4*)(p.out + off) = float4{y[0], y[1], y[2], y[3]};
        }
    }
}

template <int NT, bool MOD>
static int deform_conv_launch_as(const DConvK& k, hipStream_t st) {
    const int64_t mt = cdiv64(k.M, DC_TP);
    const int bands = cdiv(k.Cout, 64 * NT);
    ARG_CHECK(mt < (1ll << 31) && bands < 65536, "deform_conv2d: too many tiles");
    LDS_LIMIT_ONCE((int)DC_LDS, deform_conv_kernel<NT, MOD>);
    hipLaunchKernelGGL((deform_conv_kernel<NT, MOD>), dim3((unsigned)mt, (unsigned)bands), dim3(256), DC_LDS, st, k);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

int deform_conv2d_launch(const float* x, int N, int H, int W, int C, const float* om, int OC, int modulated, int stride, const float* w, int Cout,
                         const float* scale, const float* shift, const float* res, int act, float* out, hipStream_t st) {
    ARG_CHECK(N >= 0 && H >= 0 && W >= 0, "deform_conv2d: negative geometry");
    ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 512, "deform_conv2d: C must be a multiple of 32 in [32, 512]");
    ARG_CHECK(Cout > 0 && Cout % 4 == 0, "deform_conv2d: Cout must be a positive multiple of 4");
    ARG_CHECK(stride == 1 || stride == 2, "deform_conv2d: stride 1 or 2 only");
    ARG_CHECK(modulated == 0 || modulated == 1, "deform_conv2d: modulated is 0 or 1");
    ARG_CHECK(OC == (modulated ? 27 : 18), "deform_conv2d: the offset tensor has 27 channels when modulated, 18 when not");
    ARG_CHECK(act == 0 || act == 1, "deform_conv2d: act 0 or 1");
    DConvK k;
    k.N = N; k.H = H; k.W = W; k.C = C; k.OC = OC; k.stride = stride; k.Cout = Cout; k.act = act;
    k.Ho = H > 0 ? (H - 1) / stride + 1 : 0;
    k.Wo = W > 0 ? (W - 1) / stride + 1 : 0;
    const int64_t M = (int64_t)N * k.Ho * k.Wo;
    if (M == 0) return ISEGMI_OK;   // nothing to do
    ARG_CHECK(x && om && w && out, "null device pointer");
    ARG_CHECK((int64_t)N * H * W * C < (1ll << 31) && M * OC < (1ll << 31) && M + DC_TP < (1ll << 31), "deform_conv2d: input must be < 2^31 elements");
    k.cout_pad = cdiv(Cout, 128) * 128;   // rows of the packed image (isegmi_conv_packed_floats)
    ARG_CHECK((int64_t)k.cout_pad * 9 * C < (1ll << 31), "deform_conv2d: weights must be < 2^31 elements");
    k.M = (int)M;
    k.x = x; k.om = om; k.w = w; k.scale = scale; k.shift = shift; k.res = res; k.out = out;
    return modulated ? deform_conv_launch_as<1, true>(k, st) : deform_conv_launch_as<1, false>(k, st);   // 64-channel bands: see the head of the file
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_deform_conv2d(const float* d_x, int N, int H, int W, int C, const float* d_om, int OC, int modulated, int stride,
                                       const float* d_w, int Cout, const float* d_scale, const float* d_shift, const float* d_res, int act, float* d_out,
                                       void* stream) {
    return deform_conv2d_launch(d_x, N, H, W, C, d_om, OC, modulated, stride, d_w, Cout, d_scale, d_shift, d_res, act, d_out, (hipStream_t)stream);
}
