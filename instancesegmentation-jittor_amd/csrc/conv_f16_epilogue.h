// conv_f16_epilogue.h -- everything AFTER the K loop of the fp16 convolution kernels, and their host launchers, written once for both MFMA shapes
// (csrc/conv_mfma_f16.hip: v_mfma_f32_32x32x16_f16; csrc/conv_mfma_f16_m16.hip: v_mfma_f32_16x16x32_f16).  The two translation units keep their own
// kernels, K loops, fragment reads and MFMA chunks (co-compiled shape variants of one kernel template spilled, see conv_mfma_f16_m16.hip); what follows
// the K loop differs between them only in which accumulator register sits in which (row, column) of the wave tile, and that is acc_traits below.  Each
// unit instantiates these templates for its own accumulator type only.
#pragma once
#include "conv_f16.h"

namespace isegmi {

// ---- the two f16 MFMA shapes (round 5).  A wave tile of WR rows x 32 TN columns is held either as TM x TN blocks of 32 x 32 (sixteen registers each,
// v_mfma_f32_32x32x16_f16: lane (lr = lane & 31, lh = lane >> 5), register e <-> row (e & 3) + 8 (e >> 2) + 4 lh, column lr) or as NA x NC blocks of
// 16 x 16 (four registers each, v_mfma_f32_16x16x32_f16: lane (l15 = lane & 15, lq = lane >> 4), register e <-> row 4 lq + e, column l15; WR = 16 NA rows
// (48 or 64), 16 NC = 32 TN columns).  Both read their operand fragments -- 8 consecutive k per lane -- from the SAME LDS chunk images: row r's 16-B
// column c sits at slot c ^ ((r >> 1) & 7); the 32 x 32 form reads column 2 s + lh of row lr in 16-deep step s, the 16 x 16 form column 4 s + lq of row
// l15 in 32-deep step s, conflict-free for ds_read_b128 either way (every 16-lane service group meets eight distinct (r >> 1) & 7 values x two row
// parities).  The chip holds a higher clock on the 16 x 16 x 32 form in power-bound loops (MI355X_MICROARCH.md "DVFS give-back" 7;
// tools/microbench/mfma_shape.hip: 1.12-1.13x on random data at equal cycles).  The 32-term sum of one 16 x 16 x 32 instruction is bit for bit what two
// chained 32 x 32 x 16 instructions give (same microbenchmark: 0 of 204 800 elements differ), and the kernels walk K exactly as their twins do: results
// do not depend on the shape (tests/test_conv_f16_gpu.py::test_mfma_shape_does_not_change_results).
// acc_traits<accumulator array>: NA x NC blocks of RB x RB, NE registers per block, register e of a lane at (row_of(e, half(lane)), col(lane)) of its
// block (row_of's third argument is a base to add the row to) -- rows ascend with e, so an aligned strip of RB / k rows of a block row is NE / k
// consecutive registers.  SR8 / SRV: rows per LDS strip of the persistent kernels' epilogue (epi8_finish: scratch is one ring stage shared by all waves,
// so strips are short) / of conv_f16_epilogue_vec (all LDS is free).
// CODE GENERATION.  These bodies reproduce the machine code of the per-unit copies they replaced: all 31 kernels of conv_mfma_f16.hip and the five
// persistent kernels of conv_mfma_f16_m16.hip are instruction for instruction what they were (tools/asm_compare.py).  That holds only
// while (a) the strip staging and the per-pass store sequence stay written out inside the two vector epilogues -- moved into helper functions, even
// force-inlined ones, they reach the optimiser in another order and every kernel changes, some past their 128-register budget -- and (b) a block's first
// row / column keeps the association of its unit's K loop, (w NA + a) RB with 32 x 32 blocks and w WR + a RB with 16 x 16 ones (the `L::RB == 32 ?`
// selections below: same value, but the other form shares other subexpressions with the kernel and moves its register allocation).  Check with
// tools/asm_compare.py before changing either.
template <class ACC> struct acc_traits;
template <int TM_, int TN_> struct acc_traits<f32x16h[TM_][TN_]> {
    static constexpr int RB = 32, NE = 16, NA = TM_, NC = TN_, WR = 32 * TM_, TN = TN_, SR8 = 8, SRV = 32;
    static __device__ __forceinline__ int col(int lane) { return lane & 31; }
    static __device__ __forceinline__ int half(int lane) { return lane >> 5; }
    static __device__ __forceinline__ int row_of(int e, int lh, int base = 0) { return base + (e & 3) + 8 * (e >> 2) + 4 * lh; }
};
template <int NA_, int NC_> struct acc_traits<f32x4h[NA_][NC_]> {
    static constexpr int RB = 16, NE = 4, NA = NA_, NC = NC_, WR = 16 * NA_, TN = NC_ / 2, SR8 = 16, SRV = 16;
    static __device__ __forceinline__ int col(int lane) { return lane & 15; }
    static __device__ __forceinline__ int half(int lane) { return lane >> 4; }
    static __device__ __forceinline__ int row_of(int e, int lh, int base = 0) { return base + (4 * lh + e); }
};

// Shared epilogue (fp32 math): y = fmaf(acc, scale, shift) + residual -> act -> fp16 (or fp32) NHWC store.  Vector path: each wave transposes its
// fp32 tile, SRV rows at a time, through a private LDS region (all staging LDS is free by now) so that residual loads and output stores are 16 B per
// lane; strided destinations / Cout % 8 != 0 take the per-element path.  RES: a residual is added -- its 16-B loads run a rolling window of two passes
// ahead of their use (see Epi8: a load awaited on the spot also drains the previous pass's stores); without a residual no load is issued at all
// (round 2 sent a dropped out-of-range load per pass and waited for it).
template <bool RES, class ACC>
__device__ __forceinline__ void conv_f16_epilogue_vec(const ConvKH& p, ACC& acc, char* smemg, int wave, int lane, int wm, int wn, int m0, int n0) {
    typedef acc_traits<ACC> L;
    constexpr int TN = L::TN, WR = L::WR, SR = L::SRV;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int PITCH = TN * 32 + 4;
    constexpr int LPR = TN * 4, RPP = 64 / LPR, NPASS = SR / RPP, NQ = WR / RPP, D = 2 < NQ ? 2 : NQ;
    constexpr int SPB = L::RB / SR, NES = L::NE / SPB;   // strips per block row, accumulator registers per strip and block
    const int lc = L::col(lane), lh = L::half(lane);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? (const void*)p.res : (const void*)p.out), 0, RES ? p.res_bytes : 0u, 0x00020000);
    const unsigned esz = p.out_f32 ? 4u : 2u;
    float* ew = (float*)smemg + wave * SR * PITCH;
    const int er = lane / LPR, ec = (lane % LPR) * 8;
    const int co8 = n0 + wn * TN * 32 + ec;
    const bool cok8 = co8 < p.Cout;
    // pass q covers tile rows RPP q ..: a lane's offsets advance by one stride per pass; rows past M are behind the descriptors' ranges
    const unsigned rstep = (unsigned)p.Cout * (2u * RPP), ostep = (unsigned)p.out_pix_stride * esz * RPP;
    unsigned rnext = cok8 ? ((unsigned)(m0 + wm * WR + er) * (unsigned)p.Cout + (unsigned)co8) * 2u : OOB;
    unsigned onext = cok8 ? ((unsigned)(m0 + wm * WR + er) * (unsigned)p.out_pix_stride + (unsigned)co8) * esz : OOB;
    u32x4h rw[D];
    if (RES) {
#pragma unroll
        for (int q = 0; q < D; ++q) { rw[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, rnext, 0, CONV_F16_RES_AUX); rnext += rstep; }
    }
#pragma unroll
    for (int s = 0; s < WR / SR; ++s) {
#pragma unroll
        for (int b = 0; b < L::NC; ++b) {
            const int co = L::RB == 32 ? n0 + (wn * L::NC + b) * 32 + lc : n0 + wn * L::TN * 32 + b * 16 + lc;
            const bool cok = co < p.Cout;
            const float sc = (cok && p.scale) ? p.scale[co] : 1.0f;
            const float sh = (cok && p.shift) ? p.shift[co] : 0.0f;
#pragma unroll
            for (int j = 0; j < NES; ++j) ew[(L::row_of(s % SPB * NES + j, lh) - s % SPB * SR) * PITCH + b * L::RB + lc] = fmaf(acc[s / SPB][b][s % SPB * NES + j], sc, sh);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int q = s * NPASS + ps;
            const int rr = ps * RPP + er;
            const f32x4h v0 = *(const f32x4h*)(ew + rr * PITCH + ec);
            const f32x4h v1 = *(const f32x4h*)(ew + rr * PITCH + ec + 4);
            unsigned ooff;
            if (p.contiguous) { ooff = onext; onext += ostep; }
            else {
                const int m = m0 + wm * WR + q * RPP + er;
                const int ni = m / p.out_div, pi = m - ni * p.out_div;
                ooff = (m < p.M && cok8) ? (unsigned)(((int64_t)ni * p.out_img_stride + (int64_t)pi * p.out_pix_stride + co8) * esz) : OOB;
            }
            float y[8];
            if (RES) {
                const f16x8 rh = __builtin_bit_cast(f16x8, rw[q % D]);
#pragma unroll
                for (int i = 0; i < 8; ++i) y[i] = (i < 4 ? v0[i] : v1[i - 4]) + (float)rh[i];
                if (q + D < NQ) { rw[q % D] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, rnext, 0, CONV_F16_RES_AUX); rnext += rstep; }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) y[i] = i < 4 ? v0[i] : v1[i - 4];
            }
            if (p.act == 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) y[i] = y[i] > 0.0f ? y[i] : 0.0f;
            }
            if (p.out_f32) {
                u32x4h o0, o1;
#pragma unroll
                for (int i = 0; i < 4; ++i) { o0[i] = __builtin_bit_cast(unsigned, y[i]); o1[i] = __builtin_bit_cast(unsigned, y[i + 4]); }
                __builtin_amdgcn_raw_buffer_store_b128(o0, rs_out, ooff, 0, CONV_F16_OUT_AUX);
                __builtin_amdgcn_raw_buffer_store_b128(o1, rs_out, ooff >= OOB ? OOB : ooff + 16u, 0, CONV_F16_OUT_AUX);
            } else {
                f16x8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = (half_t)y[i];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4h, o), rs_out, ooff, 0, CONV_F16_OUT_AUX);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <class ACC>
__device__ __forceinline__ void conv_f16_epilogue(const ConvKH& p, ACC& acc, char* smemg, int wave, int lane, int wm, int wn, int m0, int n0) {
    typedef acc_traits<ACC> L;
    const int lc = L::col(lane), lh = L::half(lane);
    if (p.vec_epi) {  // uniform
        if (p.res) conv_f16_epilogue_vec<true>(p, acc, smemg, wave, lane, wm, wn, m0, n0);
        else conv_f16_epilogue_vec<false>(p, acc, smemg, wave, lane, wm, wn, m0, n0);
        return;
    }
    // ---- per-element path (strided destinations with Cout % 8 != 0: the RPN / prediction heads): y = fmaf(acc, scale, shift) + residual -> act; one
    // accumulator register at a time.  No LDS.
    constexpr int NA = L::NA, NC = L::NC, WR = L::WR, NE = L::NE;
    constexpr unsigned OOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(p.res ? (const void*)p.res : (const void*)p.out), 0, p.res ? p.res_bytes : 0u, 0x00020000);
    const unsigned esz = p.out_f32 ? 4u : 2u;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        unsigned rowoff[NE], resoff[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int m = L::row_of(e, lh, L::RB == 32 ? m0 + (wm * NA + a) * 32 : m0 + wm * WR + a * 16);
            resoff[e] = m < p.M ? (unsigned)m * (unsigned)p.Cout * 2u : OOB;
            if (p.contiguous) rowoff[e] = m < p.M ? (unsigned)m * (unsigned)p.out_pix_stride * esz : OOB;
            else {
                const int ni = m / p.out_div, pi = m - ni * p.out_div;
                rowoff[e] = m < p.M ? (unsigned)(((int64_t)ni * p.out_img_stride + (int64_t)pi * p.out_pix_stride) * esz) : OOB;
            }
        }
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            const int co = L::RB == 32 ? n0 + (wn * L::NC + b) * 32 + lc : n0 + wn * L::TN * 32 + b * 16 + lc;
            const bool cok = co < p.Cout;
            const float sc = (cok && p.scale) ? p.scale[co] : 1.0f;
            const float sh = (cok && p.shift) ? p.shift[co] : 0.0f;
            const unsigned cooff = cok ? (unsigned)co : OOB;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const unsigned short hb = __builtin_amdgcn_raw_buffer_load_b16(rs_res, (resoff[e] | cooff) >= OOB ? OOB : resoff[e] + cooff * 2u, 0, 0);
                float y = fmaf(acc[a][b][e], sc, sh);
                y = y + (float)__builtin_bit_cast(half_t, hb);
                y = p.act == 1 ? (y > 0.0f ? y : 0.0f) : y;
                const unsigned off = (rowoff[e] | cooff) >= OOB ? OOB : rowoff[e] + cooff * esz;
                if (p.out_f32) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rs_out, off, 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (half_t)y), rs_out, off, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The PERSISTENT kernels' epilogue (conv_f16_persist_kernel; the protocol is described at the kernel in conv_mfma_f16.hip).
// Round 3: the residual of a tile is REQUESTED BEFORE its K loop and consumed strip by strip behind a rolling window.  Before, every
// 8-row strip issued its residual load and waited for it on the spot -- and on gfx9 a wave's stores count in the same vmcnt as its loads, so
// the wait also drained the previous strip's stores: eight exposed memory round trips per 64x64 wave tile, on layers whose K loop is four
// 16-MFMA chunks (R101 res4 conv3: 14.7 % MfmaUtil at 3.9 TB/s, on neither roof).  Now the first EPI_D strips' residuals are in flight
// during the K loop (the MFMA waves issue no other vector-memory instruction there), strip q's slot is refilled with strip q + EPI_D's
// right after use, and the counted waits the compiler derives from program order never drain the stores of the strip just written.
// Offsets: a lane's residual / output offset is ONE add per strip -- lane base (its row inside the strip, its 8 channels; the out-of-range
// constant for a column past Cout) plus a wave-uniform row term; rows past M fall behind descriptors cut at M rows (contiguous
// destinations; strided ones keep the general arithmetic).
#ifndef ISEGMI_EPI_D
#define ISEGMI_EPI_D 2
#endif
constexpr int EPI_D = ISEGMI_EPI_D;   // residual passes in flight per lane (tools/build_variant.sh ... -DISEGMI_EPI_D=4 for an A/B)

template <int WR, int TN>   // WR rows x 32 TN columns per wave
struct Epi8 {
    static_assert(TN == 2 || TN == 4, "strips are 64 or 128 channels wide");
    static constexpr int LPR = TN * 4, RPP = 64 / LPR, NQ = WR / RPP;  // passes (b128 per lane) per wave tile
    // residual passes in flight per lane: a 64-row wave tile (64 accumulator registers of the 128 a wave has at 16 waves per CU) leaves room for two.
    // Round 6 tried the other end -- a 96 x 256 tile, 32-row wave tiles, ALL four passes of a wave in flight under the K loop (100 registers, no
    // spill, bit-identical) -- on R101 res4 conv3 (M = 33 600, K = 256, Cout = 1024, with residual): 45 us against 47 (tile 37) / 44 (47) alone, level
    // in the model: the residual round trips are not what bounds these layers, the CU's LDS fill path is (224 KB of A + B per 192 x 256 tile for
    // 25 MFLOP; profiles/r06_experiments.txt 2).  Not kept.
    static constexpr int D = EPI_D < NQ ? EPI_D : NQ;
    u32x4h r[D];
    unsigned rnext;   // residual offset (bytes) of the next pass to request, or >= OOB for a column past Cout; pass q covers tile rows RPP q ..
    int ux, uy, un;   // UP2X: output pixel (x, y, image) of the next pass to request
};

// UP2X (FPN top-down merge, SURVEY 8a M3: `last_inner = inner_lateral + interpolate(last_inner, scale_factor=2, mode="nearest")`): the residual of output pixel
// (n, y, x) is pixel (n, min(y >> 1, Hc - 1), min(x >> 1, Wc - 1)) of the coarser level.  A lane's pass-to-pass step is RPP pixels along the row: the walk is
// incremental (one wrap test per pass), the two divisions that start it are per tile.
template <int WR, int TN>
__device__ __forceinline__ unsigned epi8_up2x_next(const ConvKH& p, Epi8<WR, TN>& E, int co8) {
    constexpr unsigned OOB = 0x80000000u;
    int yc = E.uy >> 1, xc = E.ux >> 1;
    yc = yc > p.rHc - 1 ? p.rHc - 1 : yc;
    xc = xc > p.rWc - 1 ? p.rWc - 1 : xc;
    const unsigned off = co8 < p.Cout ? ((unsigned)((E.un * p.rHc + yc) * p.rWc + xc) * (unsigned)p.Cout + (unsigned)co8) * 2u : OOB;   // images past N are past the range
    E.ux += Epi8<WR, TN>::RPP;
    if (E.ux >= p.Wo) { E.ux -= p.Wo; E.uy += 1; if (E.uy >= p.Ho) { E.uy = 0; E.un += 1; } }
    return off;
}

// before the K loop: the first D residual passes of the wave's tile
template <int WR, int TN, bool UP2X = false>
__device__ __forceinline__ void epi8_prefetch(const ConvKH& p, Epi8<WR, TN>& E, int lane, int wm, int wn, int m0, int n0) {
    constexpr unsigned OOB = 0x80000000u;
    constexpr int LPR = Epi8<WR, TN>::LPR, RPP = Epi8<WR, TN>::RPP;
    // no branch on p.res here: a conditional prefetch makes the window a phi, and the compiler then parks the loaded registers in copies
    // behind an s_waitcnt vmcnt(0) in FRONT of the K loop; without a residual the descriptor is empty and the loads return zeros unused
    const int er = lane / LPR, ec = (lane % LPR) * 8;
    const int co8 = n0 + wn * TN * 32 + ec;
    E.rnext = co8 < p.Cout ? ((unsigned)(m0 + wm * WR + er) * (unsigned)p.Cout + (unsigned)co8) * 2u : OOB;
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(p.res ? (const void*)p.res : (const void*)p.out), 0, p.res ? p.res_bytes : 0u, 0x00020000);
    const unsigned rstep = (unsigned)p.Cout * (2u * RPP);
    if constexpr (UP2X) {
        const int m = m0 + wm * WR + er, hw = p.Ho * p.Wo;
        E.un = m / hw;
        const int rem = m - E.un * hw;
        E.uy = rem / p.Wo;
        E.ux = rem - E.uy * p.Wo;
#pragma unroll
        for (int q = 0; q < Epi8<WR, TN>::D; ++q) E.r[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, epi8_up2x_next<WR, TN>(p, E, co8), 0, CONV_F16_RES_AUX);
        return;
    }
#pragma unroll
    for (int q = 0; q < Epi8<WR, TN>::D; ++q) { E.r[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, E.rnext, 0, CONV_F16_RES_AUX); E.rnext += rstep; }
}

// SR8-row strips (registers 4g .. 4g + 3 of the 32 x 32 blocks: 8 rows; one row of 16 x 16 blocks: 16 rows); ew = the wave's SR8 x PITCH floats of scratch
template <bool RES, bool UP2X, class ACC>
__device__ __forceinline__ void epi8_finish_impl(const ConvKH& p, ACC& acc, Epi8<acc_traits<ACC>::WR, acc_traits<ACC>::TN>& E, float* ew, int lane, int wm, int wn, int m0, int n0) {
    typedef acc_traits<ACC> L;
    constexpr int TN = L::TN, WR = L::WR, SR = L::SR8, NC = L::NC;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int PITCH = TN * 32 + 4;
    constexpr int LPR = Epi8<WR, TN>::LPR, RPP = Epi8<WR, TN>::RPP, NPASS = SR / RPP, NQ = Epi8<WR, TN>::NQ, D = Epi8<WR, TN>::D;
    static_assert(WR / SR * NPASS == NQ, "passes per wave tile");
    constexpr int SPB = L::RB / SR, NES = L::NE / SPB;   // strips per block row, accumulator registers per strip and block
    const int lc = L::col(lane), lh = L::half(lane);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? (const void*)p.res : (const void*)p.out), 0, RES ? p.res_bytes : 0u, 0x00020000);
    const unsigned esz = p.out_f32 ? 4u : 2u;
    const int er = lane / LPR, ec = (lane % LPR) * 8;
    const int co8 = n0 + wn * TN * 32 + ec;
    const bool cok8 = co8 < p.Cout;
    const unsigned rstep = (unsigned)p.Cout * (2u * RPP);
    const unsigned ostep = (unsigned)p.out_pix_stride * esz * RPP;
    unsigned onext = cok8 ? ((unsigned)(m0 + wm * WR + er) * (unsigned)p.out_pix_stride + (unsigned)co8) * esz : OOB;
    float sc[NC], sh[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
            const int co = L::RB == 32 ? n0 + (wn * L::NC + b) * 32 + lc : n0 + wn * L::TN * 32 + b * 16 + lc;
        const bool cok = co < p.Cout;
        sc[b] = (cok && p.scale) ? p.scale[co] : 1.0f;
        sh[b] = (cok && p.shift) ? p.shift[co] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < WR / SR; ++s) {
#pragma unroll
        for (int b = 0; b < NC; ++b)
#pragma unroll
            for (int j = 0; j < NES; ++j) ew[(L::row_of(s % SPB * NES + j, lh) - s % SPB * SR) * PITCH + b * L::RB + lc] = fmaf(acc[s / SPB][b][s % SPB * NES + j], sc[b], sh[b]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int q = s * NPASS + ps;
            const int rr = ps * RPP + er;
            const f32x4h v0 = *(const f32x4h*)(ew + rr * PITCH + ec);
            const f32x4h v1 = *(const f32x4h*)(ew + rr * PITCH + ec + 4);
            unsigned ooff;
            if (p.contiguous) { ooff = onext; onext += ostep; }
            else {
                const int m = m0 + wm * WR + q * RPP + er;
                const int ni = m / p.out_div, pi = m - ni * p.out_div;
                ooff = (m < p.M && cok8) ? (unsigned)(((int64_t)ni * p.out_img_stride + (int64_t)pi * p.out_pix_stride + co8) * esz) : OOB;
            }
            float y[8];
            if (RES) {
                const f16x8 rh = __builtin_bit_cast(f16x8, E.r[q % D]);
                if constexpr (UP2X) {
                    // the lateral conv's result is rounded to fp16 FIRST, as the two-launch path stores it before nearest2x_add_f16 adds the coarser level
#pragma unroll
                    for (int i = 0; i < 8; ++i) y[i] = (float)(half_t)(i < 4 ? v0[i] : v1[i - 4]) + (float)rh[i];
                    if (q + D < NQ) E.r[q % D] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, epi8_up2x_next<WR, TN>(p, E, co8), 0, CONV_F16_RES_AUX);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) y[i] = (i < 4 ? v0[i] : v1[i - 4]) + (float)rh[i];
                    if (q + D < NQ) { E.r[q % D] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, E.rnext, 0, CONV_F16_RES_AUX); E.rnext += rstep; }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) y[i] = i < 4 ? v0[i] : v1[i - 4];
            }
            if (p.act == 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) y[i] = y[i] > 0.0f ? y[i] : 0.0f;
            }
            if (p.out_f32) {
                u32x4h o0, o1;
#pragma unroll
                for (int i = 0; i < 4; ++i) { o0[i] = __builtin_bit_cast(unsigned, y[i]); o1[i] = __builtin_bit_cast(unsigned, y[i + 4]); }
                __builtin_amdgcn_raw_buffer_store_b128(o0, rs_out, ooff, 0, CONV_F16_OUT_AUX);
                __builtin_amdgcn_raw_buffer_store_b128(o1, rs_out, ooff >= OOB ? OOB : ooff + 16u, 0, CONV_F16_OUT_AUX);
            } else {
                f16x8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = (half_t)y[i];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4h, o), rs_out, ooff, 0, CONV_F16_OUT_AUX);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <bool UP2X, class ACC>
__device__ __forceinline__ void epi8_finish(const ConvKH& p, ACC& acc, Epi8<acc_traits<ACC>::WR, acc_traits<ACC>::TN>& E, float* ew, int lane, int wm, int wn, int m0, int n0) {
    if constexpr (UP2X) { epi8_finish_impl<true, true>(p, acc, E, ew, lane, wm, wn, m0, n0); return; }
    if (p.res) epi8_finish_impl<true, false>(p, acc, E, ew, lane, wm, wn, m0, n0);   // uniform
    else epi8_finish_impl<false, false>(p, acc, E, ew, lane, wm, wn, m0, n0);
}

// ---------------------------------------------------------------------------------------------------------------------
// FUSED 1x1 HEAD (round 4; RPNHead under configs[4]: `t = relu(conv3x3(x)); logits, deltas = cls_logits(t), bbox_pred(t)`).  On a 192 x 256
// row-strip tile the block holds ALL 256 channels of its 192 pixels, so the 1x1 convolution that follows (256 -> f_cout <= 32 outputs: 3 objectness + 12
// box deltas) can run on the tile before it ever leaves the CU: the BN + ReLU result goes to LDS as fp16 -- rounded exactly where the two-launch path
// rounds it when it stores t -- in a row-major [pixel][256] image (16-B columns XOR-swizzled by the row), the head's packed weights (32 rows) next to
// it, and six waves multiply one 32-pixel tile each on the same 16 k-steps the stand-alone 1x1 launch would walk -- on v_mfma_f32_32x32x16_f16 whichever
// shape the 3x3 ran on.  t is never written (275 MB per P2 level at R101 bs=8) nor read back.  Bit-identical to the two launches
// (tests/test_rpn_head_f16_gpu.py).
template <class ACC>
__device__ __forceinline__ void conv_f16_epilogue_head(const ConvKH& p, ACC& acc, char* smemg, int wave, int lane, int wm, int wn, int m0) {
    typedef acc_traits<ACC> L;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int BMH = 192, T_BYTES = BMH * 512;   // the tile image; the head's weights follow it (32 rows x 512 B)
    const int lr = lane & 31, lh = lane >> 5;
    const int tid = wave * 64 + lane;                // 12 MFMA waves: 768 threads
    // head weights: rows 0..31 of the packed [128][256] image (zero rows past f_cout), 16 KB = 1024 16-B pieces
    u32x4h wv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int piece = tid + j * 768;
        wv[j] = piece < 1024 ? *(const u32x4h*)((const char*)p.f_w + piece * 16) : u32x4h{0u, 0u, 0u, 0u};
    }
    // 1. y = relu(fmaf(acc, scale, shift)) -> fp16 -> T[row][channel]
#pragma unroll
    for (int a = 0; a < L::NA; ++a)
#pragma unroll
        for (int b = 0; b < L::NC; ++b) {
            const int co = L::RB == 32 ? (wn * L::NC + b) * 32 + L::col(lane) : wn * L::TN * 32 + b * 16 + L::col(lane);
            const float sc = p.scale ? p.scale[co] : 1.0f, sh = p.shift ? p.shift[co] : 0.0f;
#pragma unroll
            for (int e = 0; e < L::NE; ++e) {
                const int row = L::row_of(e, L::half(lane), L::RB == 32 ? (wm * L::NA + a) * 32 : wm * L::WR + a * 16);
                float y = fmaf(acc[a][b][e], sc, sh);
                y = y > 0.0f ? y : 0.0f;
                *(half_t*)(smemg + row * 512 + (((co >> 3) ^ (row & 15)) << 4) + (co & 7) * 2) = (half_t)y;
            }
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int piece = tid + j * 768;
        if (piece < 1024) {
            const int row = piece >> 5, c16 = piece & 31;
            *(u32x4h*)(smemg + T_BYTES + row * 512 + ((c16 ^ (row & 15)) << 4)) = wv[j];
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the MFMA waves (the loader waves have left)
    if (wave >= BMH / 32) return;
    // 2. wave w: pixels 32 w .. + 31 of the tile x 32 head outputs, K = 256 in the order the stand-alone 1x1 launch walks it
    f32x16h h;
#pragma unroll
    for (int e = 0; e < 16; ++e) h[e] = 0.0f;
    const int prow = wave * 32 + lr;
    const char* pa = smemg + prow * 512;
    const char* pb = smemg + T_BYTES + lr * 512;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const f16x8 fa = *(const f16x8*)(pa + (((ks * 2 + lh) ^ (prow & 15)) << 4));
        const f16x8 fb = *(const f16x8*)(pb + (((ks * 2 + lh) ^ (lr & 15)) << 4));
        h = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, h, 0, 0, 0);
    }
    // 3. the head's own scale / shift, fp32 [M][f_cout] store
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.f_out, 0, p.f_out_bytes, 0x00020000);
    const bool cok = lr < p.f_cout;
    const float sc2 = (cok && p.f_scale) ? p.f_scale[lr] : 1.0f, sh2 = (cok && p.f_shift) ? p.f_shift[lr] : 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        float y = fmaf(h[e], sc2, sh2);
        y = y + 0.0f;   // the stand-alone launch's per-element epilogue adds its (absent) residual: -0 becomes +0 there, so here too
        const unsigned off = (cok && m < p.M) ? ((unsigned)m * (unsigned)p.f_cout + (unsigned)lr) * 4u : OOB;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rs, off, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  Each translation unit wraps these two with its own kernel template (launch_strip / launch_p there): KERN is the instantiation to start, ACC
// the accumulator array a wave of it holds -- its strip heights (acc_traits) size the epilogues' LDS scratch.
#ifdef ISEGMI_STRIP_TRACE
// development build only (-DISEGMI_STRIP_TRACE, tools/strip_trace.py): block 0 keeps four cycle stamps per step and wave in LDS behind the staging buffers and dumps them to p.trace
#define STRIP_TRACE(u, slot)                                                                                      \
    do {                                                                                                          \
        if (bid == 0 && (u) < 64 && !(p.dbg & 16)) {                                                              \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                           \
            *(volatile unsigned*)(smemg + TRACE_OFF + ((wave * 64 + (u)) * 4 + (slot)) * 4) = (unsigned)t_;        \
        }                                                                                                         \
    } while (0)
#else
#define STRIP_TRACE(u, slot) do {} while (0)
#endif

template <auto KERN, class ACC, int BM, int BN, int WM, int WN, int LW, int NB>
static int conv_f16_launch_strip(ConvKH& k, hipStream_t st) {
    k.mtiles = cdiv(k.M, BM);
    k.ntiles = cdiv(k.Cout, BN);
    constexpr int NW = WM * WN, TN = acc_traits<ACC>::TN, SRV = acc_traits<ACC>::SRV;
    static_assert(acc_traits<ACC>::WR * WM == BM && TN * 32 * WN == BN, "wave tile");
    size_t lds = 2 * (size_t)(BM + 64) * 128 + NB * (size_t)BN * 128;
    static_assert(2 * (BM + 64) * 128 + NB * BN * 128 <= 163840, "LDS");
    const size_t epi = (size_t)NW * SRV * (TN * 32 + 4) * 4;
    if (epi > lds) lds = epi;
    size_t lds_attr = lds;
#ifdef ISEGMI_STRIP_TRACE
    if (NB == 2) lds_attr = lds + 16384;
    static unsigned* trace_buf = nullptr;
    const bool tracing = NB == 2 && getenv("ISEGMI_STRIP_TRACE_DUMP") != nullptr;   // (NB = 3 fills the LDS: no room for the stamps)
    if (tracing) {
        lds = 2 * (size_t)(BM + 64) * 128 + NB * (size_t)BN * 128 + 16384;
        if (!trace_buf) HIP_TRY(hipMalloc((void**)&trace_buf, 16448));
        HIP_TRY(hipMemsetAsync(trace_buf, 0, 16448, st));
    }
    k.trace = tracing ? trace_buf : nullptr;
    if (tracing && getenv("ISEGMI_STRIP_TRACE_LIGHT")) k.dbg |= 16;
#endif
    LDS_LIMIT_ONCE((int)lds_attr, KERN);
    hipLaunchKernelGGL(KERN, dim3((unsigned)(k.mtiles * k.ntiles)), dim3((NW + LW) * 64), lds, st, k);
    HIP_TRY(hipGetLastError());
#ifdef ISEGMI_STRIP_TRACE
    if (tracing) {
        static unsigned host[4112];
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(host, trace_buf, 16448, hipMemcpyDeviceToHost));
        FILE* f = fopen(getenv("ISEGMI_STRIP_TRACE_DUMP"), "w");
        if (f) {
            fprintf(f, "-1 -1 %u %u 0 0\n", host[4096], host[4097]);
            for (int w = 0; w < NW + LW; ++w)
                for (int u = 0; u < 64; ++u) fprintf(f, "%d %d %u %u %u %u\n", w, u, host[(w * 64 + u) * 4], host[(w * 64 + u) * 4 + 1], host[(w * 64 + u) * 4 + 2], host[(w * 64 + u) * 4 + 3]);
            fclose(f);
        }
    }
#endif
    return ISEGMI_OK;
}

// bytes of strip scratch a persistent kernel needs BEHIND its ring: the SR8-row epilogue strips of the waves that do not fit the stage read last (at
// least the 5120 B of round 5's 144 x 256 tile, whose layout tests pin)
template <int BM, int BN, int WM, int WN, int SR8>
constexpr int p_espare() {
    constexpr int NW = WM * WN, TN = BN / WN / 32, STAGEB = (BM + BN) * 128, EWB = SR8 * (TN * 32 + 4) * 4;
    constexpr int EFIT = STAGEB / EWB < NW ? STAGEB / EWB : NW;
    constexpr int need = (NW - EFIT) * EWB;
    return need > 5120 ? (need + 1023) / 1024 * 1024 : 5120;
}

// persistent loader-wave kernel: at most one block per CU slot, each walking tiles bid, bid + grid, ...; `few` (test hook) forces
// an 8-block grid so that small test shapes exercise the multi-tile stream
template <auto KERN, class ACC, int BM, int BN, int WM, int WN, int NSTAGE, int OCC, int LW>
static int conv_f16_launch_p(ConvKH& k, hipStream_t st, bool few) {
    k.mtiles = cdiv(k.M, BM);
    k.ntiles = cdiv(k.Cout, BN);
    constexpr int NW = WM * WN, TN = acc_traits<ACC>::TN, SR8 = acc_traits<ACC>::SR8;
    static_assert(acc_traits<ACC>::WR * WM == BM && TN * 32 * WN == BN, "wave tile");
    size_t lds = (size_t)NSTAGE * (BM + BN) * 128;
    // behind the ring, only where the tile needs them: the strip scratch of the waves that do not fit the last stage, and LW KiB of landing zone for the
    // dropped pieces of a partial A round (conv_f16_persist_kernel: EFIT; conv_f16_persist_loader: issue_chunk)
    constexpr int ESPARE = p_espare<BM, BN, WM, WN, SR8>();
    constexpr bool spare = (BM / 8) % LW != 0 || NW * SR8 * (TN * 32 + 4) * 4 > (BM + BN) * 128;
    if (spare) lds += ESPARE + (size_t)LW * 1024;
    static_assert(NSTAGE * (BM + BN) * 128 + (spare ? ESPARE + LW * 1024 : 0) <= 163840, "LDS");
    LDS_LIMIT_ONCE((int)lds, KERN);
    const int ncu = device_cu_count();
    const int64_t total = (int64_t)k.mtiles * k.ntiles;
    int64_t slots = few ? 8 : (int64_t)(ncu / 8) * 8 * OCC;  // a multiple of 8, so that a block's tiles stay on its XCD
    if (slots < 8) slots = 8;
    const unsigned grid = (unsigned)(total < slots ? total : slots);
    hipLaunchKernelGGL(KERN, dim3(grid), dim3((NW + LW) * 64), lds, st, k);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi
