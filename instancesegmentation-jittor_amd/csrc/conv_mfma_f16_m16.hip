// conv_mfma_f16_m16.hip -- the fp16 backbone tiles on v_mfma_f32_16x16x32_f16 (round 5): the 192 x 256 row-strip kernel (3x3 / 1 / 1) and the
// persistent loader-wave kernel of csrc/conv_mfma_f16.hip with the SAME loaders, LDS chunk images, barrier protocol, tile walk and output tile per wave
// (64 x 64) -- only the MFMA waves' fragment reads, the instruction and the accumulator layout (hence the epilogues' staging) differ.  Its own translation
// unit so that the 32 x 32 x 16 kernels' code generation is untouched (co-compiled template variants share register-allocation context: the first attempt,
// one template with a shape parameter, spilled in the 32 x 32 x 16 instantiations that had not spilled before).  What the two forms share lives ONCE:
// the persistent kernel's loader role and the XCD-aware tile order in conv_f16.h (conv_f16_persist_loader, ConvF16TileOrder), the strip kernel's
// geometry / loader state / loader loop in conv_f16_strip_state.inc and conv_f16_strip_loader_loop.inc, and everything after the K loop -- the accumulator
// layouts (acc_traits), the three epilogues, the fused head -- with the host launchers in conv_f16_epilogue.h.  What remains here is what the shape decides
// inside the K loop: the kernels' fragment reads and the chunk of MFMAs.  The kernels' protocols are described at their twins in conv_mfma_f16.hip.
// (The template parameter MS = 1 only marks the form in the kernels' mangled names.)
#include "conv_f16_epilogue.h"

namespace isegmi {

// One 64-deep chunk on v_mfma_f32_16x16x32_f16: NA x NC blocks of 16 x 16, two 32-deep steps.  oa[i] / ob + j * 2048 = byte offsets (from sa / sb) of the
// lane's step-0 fragment of block i / j (row l15 of the block, 16-B column lq, swizzled); oa1 / ob1 = the same for step 1: the offset ^ 64 (every other
// term is a multiple of 128).  Registers: the wave tile's 64 accumulators (the kernels run four waves per SIMD: 128 registers) leave room for SIX fragment
// sets, not for the sixteen a chunk reads: the B fragments of a step stay (four sets), the A fragments go through TWO sets -- the chunk is 2 NA block rows
// (step 0's, then step 1's), row r multiplies out of set r & 1, and as soon as its MFMAs are issued the set is refilled with row r + 2's fragment: one row
// of MFMAs (64 cycles of this wave's, more with the SIMD's other waves in between) covers the read.  Step 1's B fragments replace step 0's one per MFMA
// inside step 0's last row.  sched_barrier pins this placement (left alone, hipcc sinks every reload to just in front of its first use).
template <int NA, int NC>
__device__ __forceinline__ void mfma16_chunk(f32x4h (&acc)[NA][NC], const char* sa, const int (&oa)[NA], const int (&oa1)[NA], const char* sb, int ob, int ob1) {
    static_assert(NA >= 2, "two A sets alternate over the chunk's 2 NA block rows");
    f16x8 fa[2], fb[NC];
    fa[0] = *(const f16x8*)(sa + oa[0]);
#pragma unroll
    for (int j = 0; j < NC; ++j) fb[j] = *(const f16x8*)(sb + ob + j * 2048);
    fa[1] = *(const f16x8*)(sa + oa[1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 2 * NA; ++r) {
        const int i = r % NA;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[r & 1], fb[j], acc[i][j], 0, 0, 0);
            if (r == NA - 1) fb[j] = *(const f16x8*)(sb + ob1 + j * 2048);
        }
        if (r + 2 < 2 * NA) fa[r & 1] = *(const f16x8*)(sa + (r + 2 < NA ? oa[(r + 2) % NA] : oa1[(r + 2) % NA]));
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int BM, int BN, int WM, int WN, int NSTAGE, int OCC, int LW, bool UP2X = false, int MS = 0>
__global__ __launch_bounds__((WM * WN + LW) * 64, OCC) void conv_f16_persist_kernel(const ConvKH p_arg) {
    static_assert(LW > 0 && NSTAGE >= 2 && NSTAGE <= 3, "loader waves, a 2- or 3-deep ring");
    // Kernel arguments are read where they are used, per role: taken by value the ~45 dwords of ConvKH are all loaded at entry and stay
    // live in SGPRs across both roles' loops (29 SGPR spills in round 2: the epilogue re-read its buffer descriptors with v_readlane before
    // every store group).  Each role reads the fields it needs from the kernarg segment behind an opaque copy of its address (the empty asm
    // keeps the loads from being hoisted back to the entry block); the epilogue's fields are re-read per tile, right in front of it.
    (void)p_arg;
    typedef const ConvKH __attribute__((address_space(4)))* karg_t;
    karg_t kp0 = (karg_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int p_mtiles = kp0->mtiles, p_ntiles = kp0->ntiles, p_nchunks = kp0->nchunks;
    constexpr int NW = WM * WN, NL = LW;
    static_assert(MS == 1 && (BM / WM) % 16 == 0 && BM % WM == 0, "16 x 16 x 32: a wave owns a whole number of 16-row blocks");
    constexpr int WR = BM / WM, TN = BN / WN / 32;   // rows per wave, 32-column units per wave
    // (a partial round of A pieces issues one dropped piece in its place -- see issue_chunk -- so a wave's vmcnt count stays uniform)
    constexpr int STAGEB = (BM + BN) * 128;
    constexpr int NA = WR / 16, NC = 2 * TN, NE = 4;   // accumulator blocks down / across, registers per block
    typedef f32x4h acc_t[NA][NC];
    constexpr int ESR = acc_traits<acc_t>::SR8;    // rows per epilogue strip
    constexpr int EWB = ESR * (TN * 32 + 4) * 4;   // a wave's strip scratch (bytes)
    // the epilogue's strips live in the ring stage the MFMA waves read last; where that stage is too small for all of them (144 x 256: 51 200 B for
    // twelve strips of 4352 B) the waves past EFIT take theirs from the spare LDS behind the ring (launch_p sizes it)
    constexpr int EFIT = STAGEB / EWB < NW ? STAGEB / EWB : NW;
    constexpr int ESPARE = p_espare<BM, BN, WM, WN, ESR>();   // bytes behind the ring for those waves' strips (conv_f16_launch_p sizes the same)
    extern __shared__ __attribute__((aligned(1024))) char smemg[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total = p_mtiles * p_ntiles, G = (int)gridDim.x, bid = (int)blockIdx.x;
    const ConvF16TileOrder order(total, p_ntiles);
    const int my_tiles = (total - bid + G - 1) / G;  // >= 1: the launcher never starts more blocks than tiles

    conv_f16_role_prio(wave >= NW);
    if (wave >= NW) {   // ---------------- loader waves (conv_f16.h: shared with the other MFMA shape's translation unit)
        conv_f16_persist_loader<BM, BN, NW, NL, NSTAGE, ESPARE>(kp0, smemg, wave, lane, bid, G, total, my_tiles, p_ntiles);
        return;
    }

    // ---------------- MFMA waves (K loop: tile geometry only; the epilogue reads its arguments per tile)
    const int wm = wave / WN, wn = wave % WN;
    const int a_off = wm * WR * 128;
    const int b_off = BM * 128 + wn * TN * 32 * 128;
    acc_t acc;
    const int swz16 = (lane & 15) * 128 + (((lane >> 4) ^ (((lane & 15) >> 1) & 7)) << 4);   // 16 x 16 x 32 form: 32-deep step s adds ^ (s << 6)
    auto chunk = [&](int rd) {  // run-time stage: branching over compile-time stages made hipcc copy and spill the accumulators
        const char* sb = smemg + rd * STAGEB;
        int oa[NA], oa1[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) { oa[i] = a_off + swz16 + i * 2048; oa1[i] = a_off + (swz16 ^ 64) + i * 2048; }
        mfma16_chunk<NA, NC>(acc, sb, oa, oa1, sb, b_off + swz16, b_off + (swz16 ^ 64));
    };
    int st = 0;
    for (int v = bid; v < total; v += G) {
        int m0, n0;
        order.template origin<BM, BN>(v, m0, n0);
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < NC; ++b)
#pragma unroll
                for (int e = 0; e < NE; ++e) acc[a][b][e] = 0.0f;
        Epi8<WR, TN> E;
        {
            karg_t k1 = kp0;
            asm volatile("" : "+s"(k1));
            const ConvKH& p = *(const ConvKH*)k1;
            if (p.vec_epi) epi8_prefetch<WR, TN, UP2X>(p, E, lane, wm, wn, m0, n0);  // the tile's first residual strips travel under its K loop
        }
        int last = 0;
        for (int t = 0; t < p_nchunks; ++t) {
            asm volatile("s_barrier" ::: "memory");
            chunk(st);
            last = st;
            st = st + 1 == NSTAGE ? 0 : st + 1;
        }
        asm volatile("s_barrier" ::: "memory");  // E: every MFMA wave has read the last chunk; its stage is now scratch
        karg_t k2 = kp0;
        asm volatile("" : "+s"(k2));
        const ConvKH& p = *(const ConvKH*)k2;
        if (p.vec_epi) epi8_finish<UP2X>(p, acc, E, (float*)(wave < EFIT ? smemg + last * STAGEB + wave * EWB : smemg + NSTAGE * STAGEB + (wave - EFIT) * EWB), lane, wm, wn, m0, n0);
        else conv_f16_epilogue(p, acc, smemg, wave, lane, wm, wn, m0, n0);  // per-element path: no LDS
    }
}

template <int BM, int BN, int WM, int WN, int LW, int NB = 2, int MS = 0>
__global__ __launch_bounds__((WM * WN + LW) * 64, 1) void conv3x3_f16_strip_kernel(const ConvKH p) {
    static_assert(NB == 2 || (NB == 3 && LW > 0 && (BN / 8) % LW == 0), "the three-buffer form needs loader waves and whole B piece rounds");
    constexpr int NW = WM * WN;
    constexpr int NL = LW > 0 ? LW : NW;            // waves that issue loads (LW > 0: dedicated loader waves, see above)
    static_assert(MS == 1 && (BM / WM) % 16 == 0 && BM % WM == 0, "16 x 16 x 32: a wave owns a whole number of 16-row blocks");
    constexpr int WR = BM / WM, TN = BN / WN / 32;   // rows per wave, 32-column units per wave
#include "conv_f16_strip_state.inc"   // tile geometry, loader state, issue_strip / next_group / issue_b / next_b: shared with the other MFMA shape's translation unit

    constexpr int NA = WR / 16, NC = 2 * TN, NE = 4, RBLK = 16;   // accumulator blocks down / across, registers per block, block rows
    typedef f32x4h acc_t[NA][NC];
    acc_t acc;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NC; ++b)
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[a][b][e] = 0.0f;

    // ---- fragment addressing: A rows are strip rows j(m) + s - 1 (per lane, per block row a, per tap s); the lane's row inside a block is lane & 15, its
    // 16-B column 4 ks + (lane >> 4)
    const int lr = lane & 15, lh = lane >> 4;
    int abase_s[NA][3];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int m = m0 + wm * WR + a * RBLK + lr;
        const int jm = (m - m0) + 1 + 2 * (m / W - row0);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int row = jm + s - 1;
            abase_s[a][s] = row * 128 + ((lh ^ ((row >> 1) & 7)) << 4);  // 32-deep step ks adds ^ (ks << 6)
        }
    }
    const int swzb = lr * 128 + ((lh ^ ((lr >> 1) & 7)) << 4);
    const int b_off = 2 * ABYTES + wn * TN * 32 * 128;

    // prologue: whole strip of group 0, B of step 0 (and of step 1 with three B buffers)
    if (loads) {
        issue_strip(0, 0); issue_strip(1, 0); issue_strip(2, 0);
        next_group();
        issue_b(0);
        next_b();
        if (NB == 3) { issue_b(1); next_b(); }
    }
#ifdef ISEGMI_STRIP_TRACE
    unsigned long long tr_c0 = 0, tr_r0 = 0;
    if (bid == 0) { tr_c0 = __builtin_amdgcn_s_memtime(); tr_r0 = __builtin_amdgcn_s_memrealtime(); }
#endif
    if (LW > 0) conv_f16_role_prio(wave >= NW);
#include "conv_f16_strip_loader_loop.inc"   // loader waves: the barrier sequence of the chunk loop below, loads only (shared text)
    // unrolled over two groups so that both LDS stages are compile-time terms (A buffer = gi & 1, B buffer = (gi + s) & 1, because
    // u = 3 gi + s): fragment addresses are a per-lane base plus an immediate
    for (int g0 = 0; g0 < ngroups; g0 += 2) {
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
            if (g0 + gg >= ngroups) break;  // uniform
            const char* sa = smemg + gg * ABYTES;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                STRIP_TRACE((g0 + gg) * 3 + s, 0);
                if (LW == 0) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                else asm volatile("s_barrier" ::: "memory");
                STRIP_TRACE((g0 + gg) * 3 + s, 1);
                const int ub = NB == 3 ? s : (gg + s) & 1;   // step u = 3 gi + s: u % 3 = s
                const char* sb = smemg + b_off + ub * BBYTES;
                static_assert(LW > 0, "the 16 x 16 x 32 form exists with loader waves only");
                int oa0[NA], oa1[NA];
#pragma unroll
                for (int a = 0; a < NA; ++a) { oa0[a] = abase_s[a][s]; oa1[a] = abase_s[a][s] ^ 64; }
                mfma16_chunk<NA, NC>(acc, sa, oa0, oa1, sb, swzb, swzb ^ 64);
            }
            if (LW == 0) next_group();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    STRIP_TRACE(63, 0);
    if constexpr (BM == 192 && BN == 256 && WM == 3 && WN == 4 && NB == 3) {
        if (p.f_w) { conv_f16_epilogue_head(p, acc, smemg, wave, lane, wm, wn, m0); return; }   // uniform
    }
    conv_f16_epilogue(p, acc, smemg, wave, lane, wm, wn, m0, n0);
    STRIP_TRACE(63, 1);
#ifdef ISEGMI_STRIP_TRACE
    if (bid == 0 && p.trace && wave == 0 && lane == 0) {
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        p.trace[4096] = (unsigned)(c1 - tr_c0); p.trace[4097] = (unsigned)(r1 - tr_r0);
    }
    if (bid == 0 && p.trace) for (int i = lane; i < 256; i += 64) p.trace[wave * 256 + i] = *(volatile unsigned*)(smemg + TRACE_OFF + (wave * 256 + i) * 4);
#endif
}
// the shared launchers (conv_f16_epilogue.h) with this unit's kernels and their accumulator arrays
template <int BM, int BN, int WM, int WN, int LW, int NB, int MS>
static int launch_strip(ConvKH& k, hipStream_t st) {
    return conv_f16_launch_strip<conv3x3_f16_strip_kernel<BM, BN, WM, WN, LW, NB, MS>, f32x4h[BM / WM / 16][BN / WN / 16], BM, BN, WM, WN, LW, NB>(k, st);
}
template <int BM, int BN, int WM, int WN, int NSTAGE, int OCC, int LW, bool UP2X, int MS>
static int launch_p(ConvKH& k, hipStream_t st, bool few) {
    return conv_f16_launch_p<conv_f16_persist_kernel<BM, BN, WM, WN, NSTAGE, OCC, LW, UP2X, MS>, f32x4h[BM / WM / 16][BN / WN / 16], BM, BN, WM, WN, NSTAGE, OCC, LW>(k, st, few);
}

int conv_f16_m16_launch(int tile, ConvKH& k, hipStream_t st, bool few) {
    switch (tile) {
        case 40: return launch_strip<192, 256, 3, 4, 4, 3, 1>(k, st);
        case 41: return launch_strip<144, 256, 3, 4, 4, 3, 1>(k, st);                 // 12 MFMA waves of 48 x 64: M = 33 600 (res4 at bs 8) is 234 tiles, one round
        case 46: return launch_p<144, 256, 3, 4, 3, 1, 4, false, 1>(k, st, few);      // the same rows for the 1x1 layers, three-deep ring
        case 44: return launch_p<256, 128, 4, 2, 3, 1, 4, false, 1>(k, st, few);
        case 47: return launch_p<192, 256, 3, 4, 2, 1, 4, false, 1>(k, st, few);
        case 48: return launch_p<192, 256, 3, 4, 2, 1, 4, true, 1>(k, st, few);
        case 49: return launch_p<128, 256, 2, 4, 3, 1, 4, false, 1>(k, st, few);
        default: break;
    }
    ARG_CHECK(false, "unknown 16 x 16 x 32 conv tile");
}

}  // namespace isegmi
