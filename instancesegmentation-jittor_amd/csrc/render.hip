// render.hip -- the painter: a draw list of mask tints, box outlines and keypoint dots onto a uint8 image, bit for bit what the host overlays do
// (isegmi.predictor.COCODemo.overlay / overlay_keypoints, isegmi.cli._overlay).  Stands where the reference's demo ends:
// cv2.imwrite(..., coco_demo.run_on_opencv_image(image)) and Yolact eval.py --image=in.png:out.png.
//
// Pixel-parallel: a pixel replays the whole list for itself, in the list's order, so one launch paints everything and no launch depends on another.
//   image   [H][W][3] u8, dense; the channel order is the caller's.  out may be the input (a thread reads and writes only its own pixels).
//   masks   [slots][ph][pw] u8 planes, ph >= H, pw >= W, the image in each plane's top-left corner (det.masks); a byte != 0 is "set".
//   entries i32 [D][8] = {slot (-1: none), x1, y1, x2, y2, colour = c0 | c1 << 8 | c2 << 16, flags (bit 0: outline), 0}
//   dots    i32 [Q][4] = {x, y, colour, half}
// Per pixel (x, y), every channel byte on its own:   for k < D:  mask k set here -> p = (p + c_k) >> 1;  on outline k -> p = c_k;
//                                                     then for j < Q:  |x - x_j| <= half_j and |y - y_j| <= half_j -> p = c_j.
// (p + c) >> 1 == uint8(0.5f * p + 0.5f * c) for all 65 536 byte pairs: the sum is exact in fp32 and the cast truncates.
//
// Shape: a thread owns PX = 4 consecutive pixels of one row -- 12 image bytes = 3 dwords, 4 mask bytes = 1 dword per entry; a wave is 64 such groups of
// ONE row, so everything that depends on (entry, row) -- the record, the plane address's alignment, the row's part of the outline and dot tests -- is
// wave-uniform: the records come through scalar loads and the row tests branch for the whole wave.  The kernel is bound by the D * H * W mask bytes.
// pw and ph * pw may be odd, so a plane row starts on any byte: a group that is not dword-aligned reads the two aligned dwords around it and shifts
// (both inside the mask allocation, else byte loads); the image's 12 bytes go as dwords when their address is aligned, else as bytes.
// No grid cap: one block per 256 x 4 pixel tile, refused (never clamped) past the 1-D grid limit.
#include <vector>

#include "engine.h"

namespace isegmi {

constexpr int PAINT_MAX_ENTRIES = 1024, PAINT_MAX_DOTS = 32768, PAINT_MAX_HALF = 8;
constexpr int PAINT_PX = 4, PAINT_BX = 64, PAINT_BY = 4;   // pixels per thread; threads per block along x (one wave) and rows per block

struct PaintK {
    const uint8_t* in; uint8_t* out;
    const uint8_t* masks; const uint8_t* masks_end;
    const int32_t* entries; const int32_t* dots;
    int H, W, slots, ph, pw, D, Q, groups_x;   // groups_x: blocks per row tile
};

// the 4 mask bytes of pixels x0 .. x0 + 3 at a (byte j in bits 8j); nv < 4: only the first nv pixels exist (the others read as 0)
__device__ __forceinline__ uint32_t paint_mask4(const uint8_t* a, int nv, const uint8_t* lo_lim, const uint8_t* hi_lim) {
    if (nv == PAINT_PX) {
        const uint32_t mis = (uint32_t)((uintptr_t)a & 3);
        if (mis == 0) return *(const uint32_t*)a;
        const uint8_t* lo = a - mis;
        if (lo >= lo_lim && lo + 8 <= hi_lim) {
            const uint32_t d0 = ((const uint32_t*)lo)[0], d1 = ((const uint32_t*)lo)[1];
            return (d0 >> (8 * mis)) | (d1 << (32 - 8 * mis));
        }
    }
    uint32_t m = 0;
    for (int j = 0; j < nv; ++j) m |= (uint32_t)a[j] << (8 * j);
    return m;
}

__global__ __launch_bounds__(PAINT_BX* PAINT_BY) void paint_kernel(const PaintK p) {
    const int bx = (int)(blockIdx.x % (unsigned)p.groups_x), by = (int)(blockIdx.x / (unsigned)p.groups_x);
    const int y = by * PAINT_BY + (int)threadIdx.y;
    const int x0 = (bx * PAINT_BX + (int)threadIdx.x) * PAINT_PX;
    if (y >= p.H || x0 >= p.W) return;
    const int nv = p.W - x0 < PAINT_PX ? p.W - x0 : PAINT_PX;
    const int64_t pix = (int64_t)y * p.W + x0;

    uint32_t px[PAINT_PX] = {0u, 0u, 0u, 0u};   // one pixel per register: c0 | c1 << 8 | c2 << 16
    const uint8_t* ia = p.in + pix * 3;
    if (nv == PAINT_PX && ((uintptr_t)ia & 3) == 0) {
        const uint32_t w0 = ((const uint32_t*)ia)[0], w1 = ((const uint32_t*)ia)[1], w2 = ((const uint32_t*)ia)[2];
        px[0] = w0 & 0xFFFFFFu;
        px[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
        px[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
        px[3] = w2 >> 8;
    } else {
        for (int j = 0; j < nv; ++j) px[j] = (uint32_t)ia[3 * j] | ((uint32_t)ia[3 * j + 1] << 8) | ((uint32_t)ia[3 * j + 2] << 16);
    }

    const int64_t plane = (int64_t)p.ph * p.pw, row_off = (int64_t)y * p.pw + x0;
    for (int k = 0; k < p.D; ++k) {   // painter's order: a dependent chain per pixel
        const int32_t* e = p.entries + 8 * k;   // wave-uniform
        const int slot = e[0], x1 = e[1], y1 = e[2], x2 = e[3], y2 = e[4], flags = e[6];
        const uint32_t c = (uint32_t)e[5] & 0xFFFFFFu;
        if ((unsigned)slot < (unsigned)p.slots) {
            const uint32_t m = paint_mask4(p.masks + slot * plane + row_off, nv, p.masks, p.masks_end);
#pragma unroll
            for (int j = 0; j < PAINT_PX; ++j) {
                const uint32_t avg = (px[j] & c) + (((px[j] ^ c) & 0xFEFEFEu) >> 1);   // per byte floor((p + c) / 2), no carry between bytes
                px[j] = ((m >> (8 * j)) & 0xFFu) ? avg : px[j];
            }
        }
        if (flags & 1) {
            const bool row_in = y1 <= y && y <= y2, row_edge = y == y1 || y == y2;
            if (row_in || row_edge) {
#pragma unroll
                for (int j = 0; j < PAINT_PX; ++j) {
                    const int x = x0 + j;
                    const bool on = (row_in && (x == x1 || x == x2)) || (row_edge && x1 <= x && x <= x2);
                    px[j] = on ? c : px[j];
                }
            }
        }
    }
    for (int q = 0; q < p.Q; ++q) {
        const int32_t* d = p.dots + 4 * q;   // wave-uniform
        const int dx = d[0], dy = d[1], half = d[3];
        const int ry = y - dy;
        if (ry > half || -ry > half) continue;   // the row misses the dot: the whole wave skips it
        const uint32_t c = (uint32_t)d[2] & 0xFFFFFFu;
#pragma unroll
        for (int j = 0; j < PAINT_PX; ++j) {
            const int rx = x0 + j - dx;
            px[j] = (rx <= half && -rx <= half) ? c : px[j];
        }
    }

    uint8_t* oa = p.out + pix * 3;
    if (nv == PAINT_PX && ((uintptr_t)oa & 3) == 0) {
        ((uint32_t*)oa)[0] = px[0] | (px[1] << 24);
        ((uint32_t*)oa)[1] = (px[1] >> 8) | (px[2] << 16);
        ((uint32_t*)oa)[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int j = 0; j < nv; ++j) {
            oa[3 * j] = (uint8_t)px[j];
            oa[3 * j + 1] = (uint8_t)(px[j] >> 8);
            oa[3 * j + 2] = (uint8_t)(px[j] >> 16);
        }
    }
}

// everything that can be refused without reading a list
static int paint_check_shape(const uint8_t* d_image, int H, int W, const uint8_t* d_masks, int slots, int ph, int pw, const void* entries, int D,
                             const void* dots, int Q, const uint8_t* d_out) {
    ARG_CHECK(d_image && d_out, "paint: null image");
    ARG_CHECK(H >= 1 && W >= 1, "paint: H, W >= 1");
    ARG_CHECK(D >= 0 && D <= PAINT_MAX_ENTRIES, "paint: 0 <= D <= 1024");
    ARG_CHECK(Q >= 0 && Q <= PAINT_MAX_DOTS, "paint: 0 <= Q <= 32768");
    ARG_CHECK((D == 0 || entries) && (Q == 0 || dots), "paint: a list with entries is not null");
    if (d_masks) {
        ARG_CHECK(slots >= 1, "paint: masks without slots");
        ARG_CHECK(ph >= H && pw >= W, "paint: the image does not fit the mask planes (ph >= H, pw >= W)");
    }
    const int64_t blocks = cdiv64(cdiv64(W, PAINT_PX), PAINT_BX) * cdiv64(H, PAINT_BY);
    ARG_CHECK(blocks <= 0x7FFFFFFFll, "paint: image larger than the grid");
    return ISEGMI_OK;
}

// the lists themselves (host copies): slots in -1 .. slots-1 (a slot needs masks), half in 0 .. 8
static int paint_check_lists(bool have_masks, int slots, const int32_t* h_entries, int D, const int32_t* h_dots, int Q) {
    for (int k = 0; k < D; ++k) {
        const int s = h_entries[8 * k];
        ARG_CHECK(s >= -1 && (s < 0 || !have_masks || s < slots), "paint: entry slot outside -1 .. slots-1");
        ARG_CHECK(s < 0 || have_masks, "paint: an entry names a slot and there are no masks");
    }
    for (int q = 0; q < Q; ++q) ARG_CHECK(h_dots[4 * q + 3] >= 0 && h_dots[4 * q + 3] <= PAINT_MAX_HALF, "paint: dot half outside 0 .. 8");
    return ISEGMI_OK;
}

// lists already checked (paint_check_shape + paint_check_lists)
static int paint_launch(const uint8_t* d_image, int H, int W, const uint8_t* d_masks, int slots, int ph, int pw, const int32_t* d_entries, int D,
                        const int32_t* d_dots, int Q, uint8_t* d_out, hipStream_t st) {
    PaintK p;
    p.in = d_image; p.out = d_out;
    p.masks = d_masks; p.masks_end = d_masks ? d_masks + (int64_t)slots * ph * pw : nullptr;
    p.entries = d_entries; p.dots = d_dots;
    p.H = H; p.W = W; p.slots = d_masks ? slots : 0; p.ph = ph; p.pw = pw; p.D = D; p.Q = Q;
    p.groups_x = cdiv(cdiv(W, PAINT_PX), PAINT_BX);
    const unsigned blocks = (unsigned)p.groups_x * (unsigned)cdiv(H, PAINT_BY);
    hipLaunchKernelGGL(paint_kernel, dim3(blocks), dim3(PAINT_BX, PAINT_BY), 0, st, p);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

// isegmi_engine_paint: the lists come from the host (checked there, staged through the pinned ring), the masks are det.masks of image_index
int eng_paint(Engine& e, int image_index, const uint8_t* d_image, int H, int W, const int32_t* h_entries, int D, const int32_t* h_dots, int Q, uint8_t* d_out) {
    TRY(paint_check_shape(d_image, H, W, nullptr, 0, 0, 0, h_entries, D, h_dots, Q, d_out));
    const int N = e.last_N;
    if (N <= 0) { set_error("paint before forward"); return ISEGMI_ERR_STATE; }
    ARG_CHECK(image_index >= 0 && image_index < N, "paint: image_index inside the last forward's batch");
    bool wants_mask = false;
    for (int k = 0; k < D; ++k) wants_mask = wants_mask || h_entries[8 * k] >= 0;
    const uint8_t* masks = nullptr;
    int K = 0, ph = 0, pw = 0;
    if (wants_mask) {
        auto mit = e.bufs.find("det.masks");
        const bool mask_engine = e.kind == 1 || e.kind == 3 || (e.kind == 2 && maskrcnn_mask_on(e));
        if (!mask_engine) { set_error("paint: an entry names a mask slot and the engine has no det.masks (box-only: paint with slot -1)"); return ISEGMI_ERR_STATE; }
        if (mit == e.bufs.end() || mit->second.d == nullptr || mit->second.shape.size() != 4 || mit->second.shape[0] != N) {
            set_error("paint: an entry names a mask slot and there is no det.masks of this batch: run postprocess / paste first");
            return ISEGMI_ERR_STATE;
        }
        if (e.kind != 3 && e.param("sparse_masks", 0.0f) != 0.0f) { set_error("paint: sparse_masks is set: det.masks holds box windows, not whole planes"); return ISEGMI_ERR_STATE; }
        K = (int)mit->second.shape[1]; ph = (int)mit->second.shape[2]; pw = (int)mit->second.shape[3];
        masks = (const uint8_t*)mit->second.d + (int64_t)image_index * K * ph * pw;
        TRY(paint_check_shape(d_image, H, W, masks, K, ph, pw, h_entries, D, h_dots, Q, d_out));
    }
    TRY(paint_check_lists(masks != nullptr, K, h_entries, D, h_dots, Q));
    hipStream_t rs = eng_results_stream(e);   // the stream that produced det.masks: the launch is ordered behind the paste / postprocess
    void *de = nullptr, *dd = nullptr;
    const auto stage = [&](const int32_t* src, int64_t bytes, void* dst) -> int {   // the ring's slots are small: a long list goes in pieces, in stream order
        for (int64_t off = 0; off < bytes; off += Engine::PIN_SLOT_BYTES) {
            const int64_t n = bytes - off < Engine::PIN_SLOT_BYTES ? bytes - off : Engine::PIN_SLOT_BYTES;
            TRY(eng_stage_small(e, (const char*)src + off, (size_t)n, (char*)dst + off, rs));
        }
        return ISEGMI_OK;
    };
    if (D > 0) {
        TRY(eng_buf(e, "paint.entries", (int64_t)PAINT_MAX_ENTRIES * 32, &de, 1, {D, 8}));
        TRY(stage(h_entries, (int64_t)D * 32, de));
    }
    if (Q > 0) {
        TRY(eng_buf(e, "paint.dots", (int64_t)Q * 16, &dd, 1, {Q, 4}));
        TRY(stage(h_dots, (int64_t)Q * 16, dd));
    }
    {
        OpScope op(e, rs, "paint (masks, outlines, dots: one pixel-parallel launch)", (double)H * W * 6 + (wants_mask ? (double)D * H * W : 0.0));
        TRY(paint_launch(d_image, H, W, masks, K, ph, pw, (const int32_t*)de, D, (const int32_t*)dd, Q, d_out, rs));
    }
    if (rs == e.tail && e.tail) HIP_TRY(hipEventRecord(e.tail_done, e.tail));   // reads det.masks: extend the WAR fence
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_op_paint(const uint8_t* d_image, int H, int W, const uint8_t* d_masks, int slots, int ph, int pw, const int32_t* d_entries, int D,
                               const int32_t* d_dots, int Q, uint8_t* d_out, void* stream) {
    TRY(paint_check_shape(d_image, H, W, d_masks, slots, ph, pw, d_entries, D, d_dots, Q, d_out));
    hipStream_t st = (hipStream_t)stream;
    // the lists live on the device and a bad slot would index outside the planes: they are read back and checked before anything is launched
    std::vector<int32_t> he((size_t)D * 8), hd((size_t)Q * 4);
    if (D > 0) HIP_TRY(hipMemcpyAsync(he.data(), d_entries, (size_t)D * 32, hipMemcpyDeviceToHost, st));
    if (Q > 0) HIP_TRY(hipMemcpyAsync(hd.data(), d_dots, (size_t)Q * 16, hipMemcpyDeviceToHost, st));
    if (D > 0 || Q > 0) HIP_TRY(hipStreamSynchronize(st));
    TRY(paint_check_lists(d_masks != nullptr, slots, he.data(), D, hd.data(), Q));
    return paint_launch(d_image, H, W, d_masks, slots, ph, pw, d_entries, D, d_dots, Q, d_out, st);
}

extern "C" int isegmi_engine_paint(isegmi_engine* h, int image_index, const uint8_t* d_image, int H, int W, const int32_t* h_entries, int D,
                                   const int32_t* h_dots, int Q, uint8_t* d_out) {
    ARG_CHECK(h, "null");
    return eng_paint(h->e, image_index, d_image, H, W, h_entries, D, h_dots, Q, d_out);
}
