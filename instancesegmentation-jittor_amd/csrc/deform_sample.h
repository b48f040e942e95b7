// deform_sample.h -- the sampling arithmetic of the deformable convolutions, in ONE place: what deform_im2col_kernel (spatial.hip) writes into the
// columns and what deform_conv_kernel (deform_conv.hip) gathers straight into its MFMA operand tile.  Oracle: ora_deform_im2col, same rounding
// sequence.  Every operation below is one rounded fp32 operation (the library is built with -ffp-contract=off); the two kernels agree bit for bit
// because neither has a copy of its own.
#pragma once
#include "detmath.h"

namespace isegmi {

// One (output pixel, tap) sampling position: the four corner weights, the mask factor, the low corner and which of the four corners lie in the image.
struct DeformTap {
    float w1, w2, w3, w4;   // (hl, wl), (hl, wl + 1), (hl + 1, wl), (hl + 1, wl + 1)
    float m;                // dm_sigmoid(mask logit); unused by the unmodulated form
    int hl, wl;
    unsigned live;          // bit c: corner c + 1 is inside the image; bit 4: the position itself is (h > -1, w > -1, h < H, w < W).  0 samples +0.
};
constexpr unsigned DEFORM_INSIDE = 16u;

// (h, w): the tap's base position plus its offset.  A position outside (-1, H) x (-1, W) -- NaN included, every comparison is false -- is dead.
__device__ __forceinline__ void deform_tap(const float h, const float w, const int H, const int W, const float logit, const bool modulated, DeformTap& t) {
    t.w1 = t.w2 = t.w3 = t.w4 = 0.0f; t.m = 0.0f; t.hl = t.wl = 0; t.live = 0u;
    if (h > -1.0f && w > -1.0f && h < (float)H && w < (float)W) {
        if (modulated) t.m = dm_sigmoid(logit);
        const float hf = floorf(h), wf = floorf(w);
        t.hl = (int)hf; t.wl = (int)wf;
        const int hh_ = t.hl + 1, wh_ = t.wl + 1;
        const float lh = h - hf, lw = w - wf, hh = 1.0f - lh, hw = 1.0f - lw;
        t.w1 = hh * hw; t.w2 = hh * lw; t.w3 = lh * hw; t.w4 = lh * lw;
        t.live = DEFORM_INSIDE | (t.hl >= 0 && t.wl >= 0 ? 1u : 0u) | (t.hl >= 0 && wh_ <= W - 1 ? 2u : 0u) | (hh_ <= H - 1 && t.wl >= 0 ? 4u : 0u) |
                 (hh_ <= H - 1 && wh_ <= W - 1 ? 8u : 0u);
    }
}

// One channel of a live position: v1..v4 are the corner values (+0 for a corner outside the image).  ((w1 v1 + w2 v2) + w3 v3) + w4 v4, then the mask.
__device__ __forceinline__ float deform_mix(const float w1, const float w2, const float w3, const float w4, const float m, const bool modulated,
                                            const float v1, const float v2, const float v3, const float v4) {
    const float v = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4;
    return modulated ? v * m : v;
}

}  // namespace isegmi
