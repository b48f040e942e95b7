// groupnorm.hip -- GroupNorm over NHWC fp32 (maskrcnn-benchmark's gn_baselines: backbone, FPN, Xconv1fc box head, mask head).
//
//   y = (x - mu) * rsqrt(var + eps) * gamma + beta  [+ residual]  [ReLU],   mu / biased var over (H, W, C / groups) of one image (or RoI) and group.
//
// GEOMETRY (both regimes).  The C channels are cut into column tiles of TW = min(C, 64) channels (a tile holds whole groups: TW % (C / groups) == 0).
// A block of 256 threads works on one tile of a run of pixels as rows x ncol threads, ncol = TW / 4, rows = 256 / ncol: thread (r, q) owns the four
// channels of float4 slot q and the pixels p0 + r, p0 + r + rows, p0 + r + 2 rows ...  A wavefront therefore reads whole 256-byte row segments with
// 16-byte loads.
//
// VARIANCE: SHIFTED DATA.  Plain fp32 E[x^2] - mu^2 cancels when |mu| >> sigma.  Every value is first shifted by the group's pivot
// K = x[n][pixel 0][first channel of the group]: d = x - K (exact when x and K lie within a factor of two of each other, one rounding otherwise), and the
// sums run over d and d * d.  |mean(d)| is then of the order of sigma whatever the offset of the data, so var = E[d^2] - mean(d)^2, taken in fp64,
// loses nothing that matters.  The apply pass also works on d: y = ((d - m) * rstd) * gamma + beta with m = fp32(mean(d)), rstd = fp32(1 / sqrt(var + eps)),
// var clamped at 0 (a NaN variance clamps to 0 as well; the group's outputs are NaN through m).
//
// SUMMATION ORDER (fixed; no atomics; tests/groupnorm_ref.py restates it in numpy and the GPU tests compare bits):
//   1. thread (r, q), per channel: fp32 chains s1 += d, s2 += d * d from +0 over its pixels in ascending order (at most 32 pixels in the large-plane
//      regime, at most 13 in the slab regime);
//   2. per channel of the tile, fp64: the chain over r = 0 .. rows-1 of the threads' (s1, s2), from +0;
//   3. per group, fp64: the chain over the group's channels in ascending order of the results of 2, from +0;
//   large planes only (a plane is cut into chunks of rows * 32 pixels, one block per chunk and tile; step 3 is the chunk's partial):
//   4. per (image, group), fp64, 64 lanes: lane l chains the partials of chunks l, l + 64, l + 128 ... from +0;
//   5. the 64 lane sums fold as a tree: for off = 32, 16, .. 1: s[l] += s[l + off] for l < off;
//   then mean(d) = S1 / count, var = S2 / count - mean(d)^2 in fp64, count = H * W * C / groups.
//
// REGIMES, chosen from the shape alone (groupnorm_is_slab): H * W <= 196 -- the RoI heads' 7x7 and 14x14 slabs, and small backbone planes -- runs ONE
// kernel: a block keeps its (slab, tile) in registers (at most 13 float4 per thread) between the statistics and the apply, x is read once and y written
// once.  Larger planes run three launches: gn_stats (reads x once, writes the per-chunk partials of step 3), gn_finalize (steps 4-5, one wavefront per
// (image, group): writes K, m, rstd) and gn_apply (reads x [+ residual], writes y).  In place (out == x, and residual == out) is allowed in both: every
// element is read and written by the same thread, and the pivot K reaches the apply pass through the statistics buffer, not through x.
#include "engine.h"

namespace isegmi {

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_TILE_C = 64;        // channels per column tile
constexpr int GN_CHUNK_ITERS = 32;   // pixels per thread and chunk (large planes)
constexpr int GN_SLAB_HW = 196;      // H * W up to which a plane is a slab (14 x 14)
constexpr int GN_SLAB_ITERS = 13;    // ceil(196 / 16): rows >= 16 because ncol <= 16

struct GnGeom {
    int C, cpg, groups, TW, ncol, rows, ntiles, HW;
};

// steps 2 and 3 for the block's tile: p1 / p2 [rows][TW] hold the threads' fp32 sums; on return g1 / g2 [TW / cpg] hold the groups' fp64 sums
__device__ __forceinline__ void gn_block_reduce(const GnGeom& g, float* p1, float* p2, double* c1, double* c2, double* g1, double* g2) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < g.TW) {
        double a = 0.0, b = 0.0;
        for (int r = 0; r < g.rows; ++r) {
            a += (double)p1[r * g.TW + t];
            b += (double)p2[r * g.TW + t];
        }
        c1[t] = a;
        c2[t] = b;
    }
    __syncthreads();
    if (t < g.TW / g.cpg) {
        double a = 0.0, b = 0.0;
        for (int c = 0; c < g.cpg; ++c) {
            a += c1[t * g.cpg + c];
            b += c2[t * g.cpg + c];
        }
        g1[t] = a;
        g2[t] = b;
    }
    __syncthreads();
}

__device__ __forceinline__ void gn_moments(double S1, double S2, double count, float eps, float* m, float* rstd) {
    const double md = S1 / count;
    double var = S2 / count - md * md;
    var = var > 0.0 ? var : 0.0;
    *m = (float)md;
    *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ float4 gn_affine(float4 v, const float* K, const float* m, const float* rs, float4 ga, float4 be, bool has_res, float4 r, int relu) {
    float4 y;
    y.x = ((v.x - K[0]) - m[0]) * rs[0] * ga.x + be.x;
    y.y = ((v.y - K[1]) - m[1]) * rs[1] * ga.y + be.y;
    y.z = ((v.z - K[2]) - m[2]) * rs[2] * ga.z + be.z;
    y.w = ((v.w - K[3]) - m[3]) * rs[3] * ga.w + be.w;
    if (has_res) {
        y.x += r.x; y.y += r.y; y.z += r.z; y.w += r.w;
    }
    if (relu) {
        y.x = y.x > 0.0f ? y.x : 0.0f; y.y = y.y > 0.0f ? y.y : 0.0f;
        y.z = y.z > 0.0f ? y.z : 0.0f; y.w = y.w > 0.0f ? y.w : 0.0f;
    }
    return y;
}

// ---- slab regime: one launch, block = (slab, tile)
__global__ void __launch_bounds__(GN_THREADS) gn_slab_kernel(const float* x, GnGeom g, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, const float* res, int relu, float* out) {
    __shared__ float p1[GN_THREADS * 4], p2[GN_THREADS * 4];
    __shared__ double c1[GN_TILE_C], c2[GN_TILE_C], g1[GN_TILE_C], g2[GN_TILE_C];
    __shared__ float sm[GN_TILE_C], sr[GN_TILE_C];
    const int t = threadIdx.x, r = t / g.ncol, q = t - r * g.ncol;
    const int64_t slab = blockIdx.x / g.ntiles;
    const int tile = blockIdx.x - (int)(slab * g.ntiles);
    const bool active = r < g.rows;
    const int ch = tile * g.TW + q * 4;   // first of the thread's four channels
    const int64_t base = slab * g.HW * g.C;
    float K[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 v[GN_SLAB_ITERS];
    float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) K[j] = x[base + ((ch + j) / g.cpg) * g.cpg];
#pragma unroll
        for (int k = 0; k < GN_SLAB_ITERS; ++k) {
            const int p = r + k * g.rows;
            if (p < g.HW) v[k] = *(const float4*)(x + base + (int64_t)p * g.C + ch);
        }
#pragma unroll
        for (int k = 0; k < GN_SLAB_ITERS; ++k) {
            const int p = r + k * g.rows;
            if (p < g.HW) {
                const float d0 = v[k].x - K[0], d1 = v[k].y - K[1], d2 = v[k].z - K[2], d3 = v[k].w - K[3];
                s1[0] += d0; s1[1] += d1; s1[2] += d2; s1[3] += d3;
                s2[0] += d0 * d0; s2[1] += d1 * d1; s2[2] += d2 * d2; s2[3] += d3 * d3;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p1[r * g.TW + q * 4 + j] = s1[j];
            p2[r * g.TW + q * 4 + j] = s2[j];
        }
    }
    gn_block_reduce(g, p1, p2, c1, c2, g1, g2);
    if (t < g.TW / g.cpg) gn_moments(g1[t], g2[t], (double)g.HW * g.cpg, eps, &sm[t], &sr[t]);
    __syncthreads();
    if (!active) return;
    float m[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gl = (q * 4 + j) / g.cpg;
        m[j] = sm[gl];
        rs[j] = sr[gl];
    }
    const float4 ga = *(const float4*)(gamma + ch), be = *(const float4*)(beta + ch);
#pragma unroll
    for (int k = 0; k < GN_SLAB_ITERS; ++k) {
        const int p = r + k * g.rows;
        if (p < g.HW) {
            const int64_t o = base + (int64_t)p * g.C + ch;
            float4 rv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (res) rv = *(const float4*)(res + o);
            *(float4*)(out + o) = gn_affine(v[k], K, m, rs, ga, be, res != nullptr, rv, relu);
        }
    }
}

// ---- large planes: block = (image, chunk, tile).  part [N][nchunks][groups][2] fp64.
__global__ void __launch_bounds__(GN_THREADS) gn_stats_kernel(const float* __restrict__ x, GnGeom g, int nchunks, double* __restrict__ part) {
    __shared__ float p1[GN_THREADS * 4], p2[GN_THREADS * 4];
    __shared__ double c1[GN_TILE_C], c2[GN_TILE_C], g1[GN_TILE_C], g2[GN_TILE_C];
    const int t = threadIdx.x, r = t / g.ncol, q = t - r * g.ncol;
    const int tile = blockIdx.x % g.ntiles;
    const int64_t nc = blockIdx.x / g.ntiles;   // image * nchunks + chunk
    const int64_t n = nc / nchunks;
    const int chunk = (int)(nc - n * nchunks);
    const int ch = tile * g.TW + q * 4;
    const int64_t base = n * g.HW * g.C;
    if (r < g.rows) {
        float K[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) K[j] = x[base + ((ch + j) / g.cpg) * g.cpg];
        float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int p0 = chunk * g.rows * GN_CHUNK_ITERS + r;
#pragma unroll 8
        for (int k = 0; k < GN_CHUNK_ITERS; ++k) {
            const int p = p0 + k * g.rows;
            if (p < g.HW) {
                const float4 v = *(const float4*)(x + base + (int64_t)p * g.C + ch);
                const float d0 = v.x - K[0], d1 = v.y - K[1], d2 = v.z - K[2], d3 = v.w - K[3];
                s1[0] += d0; s1[1] += d1; s1[2] += d2; s1[3] += d3;
                s2[0] += d0 * d0; s2[1] += d1 * d1; s2[2] += d2 * d2; s2[3] += d3 * d3;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p1[r * g.TW + q * 4 + j] = s1[j];
            p2[r * g.TW + q * 4 + j] = s2[j];
        }
    }
    gn_block_reduce(g, p1, p2, c1, c2, g1, g2);
    const int gpt = g.TW / g.cpg;   // groups per tile
    if (t < gpt) {
        double* o = part + (nc * g.groups + (int64_t)tile * gpt + t) * 2;
        o[0] = g1[t];
        o[1] = g2[t];
    }
}

// one wavefront per (image, group): stat [N * groups][4] = {K, m, rstd, 0}
__global__ void __launch_bounds__(64) gn_finalize_kernel(const float* __restrict__ x, GnGeom g, int nchunks, const double* __restrict__ part, float eps,
                                                         float* __restrict__ stat) {
    __shared__ double a1[64], a2[64];
    const int l = threadIdx.x;
    const int64_t ng = blockIdx.x, n = ng / g.groups;
    const int grp = (int)(ng - n * g.groups);
    double s1 = 0.0, s2 = 0.0;
    for (int c = l; c < nchunks; c += 64) {
        const double* pp = part + ((n * nchunks + c) * g.groups + grp) * 2;
        s1 += pp[0];
        s2 += pp[1];
    }
    a1[l] = s1;
    a2[l] = s2;
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) {
        if (l < off) {
            a1[l] += a1[l + off];
            a2[l] += a2[l + off];
        }
        __syncthreads();
    }
    if (l == 0) {
        float m, rs;
        gn_moments(a1[0], a2[0], (double)g.HW * g.cpg, eps, &m, &rs);
        float* o = stat + ng * 4;
        o[0] = x[n * g.HW * g.C + grp * g.cpg];
        o[1] = m;
        o[2] = rs;
        o[3] = 0.0f;
    }
}

__global__ void __launch_bounds__(GN_THREADS) gn_apply_kernel(const float* x, GnGeom g, int nchunks, const float* __restrict__ stat,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, const float* res, int relu,
                                                              float* out) {
    const int t = threadIdx.x, r = t / g.ncol, q = t - r * g.ncol;
    if (r >= g.rows) return;
    const int tile = blockIdx.x % g.ntiles;
    const int64_t nc = blockIdx.x / g.ntiles;
    const int64_t n = nc / nchunks;
    const int chunk = (int)(nc - n * nchunks);
    const int ch = tile * g.TW + q * 4;
    const int64_t base = n * g.HW * g.C;
    float K[4], m[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* s = stat + (n * g.groups + (ch + j) / g.cpg) * 4;
        K[j] = s[0];
        m[j] = s[1];
        rs[j] = s[2];
    }
    const float4 ga = *(const float4*)(gamma + ch), be = *(const float4*)(beta + ch);
    const int p0 = chunk * g.rows * GN_CHUNK_ITERS + r;
#pragma unroll 8
    for (int k = 0; k < GN_CHUNK_ITERS; ++k) {
        const int p = p0 + k * g.rows;
        if (p < g.HW) {
            const int64_t o = base + (int64_t)p * g.C + ch;
            const float4 v = *(const float4*)(x + o);
            float4 rv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (res) rv = *(const float4*)(res + o);
            *(float4*)(out + o) = gn_affine(v, K, m, rs, ga, be, res != nullptr, rv, relu);
        }
    }
}

int gn_geometry(int64_t N, int H, int W, int C, int groups, GnGeom* g) {
    ARG_CHECK(N >= 0 && H > 0 && W > 0 && C > 0 && groups > 0, "group_norm: shape");
    ARG_CHECK(C % 4 == 0, "group_norm: C must be a multiple of 4");
    ARG_CHECK(C % groups == 0, "group_norm: groups must divide C");
    ARG_CHECK((int64_t)H * W < (int64_t)1 << 30, "group_norm: plane too large");
    g->C = C; g->groups = groups; g->cpg = C / groups; g->HW = H * W;
    g->TW = C < GN_TILE_C ? C : GN_TILE_C;
    ARG_CHECK(C % g->TW == 0 && g->TW % g->cpg == 0, "group_norm: a 64-channel tile must hold whole groups (C % 64 == 0 and 64 % (C / groups) == 0, or C < 64)");
    g->ncol = g->TW / 4;
    g->rows = GN_THREADS / g->ncol;
    g->ntiles = C / g->TW;
    return ISEGMI_OK;
}

int64_t gn_chunks(const GnGeom& g) { return cdiv64(g.HW, (int64_t)g.rows * GN_CHUNK_ITERS); }

}  // namespace

bool groupnorm_is_slab(int H, int W) { return (int64_t)H * W <= GN_SLAB_HW; }

// workspace of the large-plane regime (0 for slabs): the chunk partials, then the per-(image, group) statistics
int64_t groupnorm_workspace_bytes(int64_t N, int H, int W, int C, int groups) {
    GnGeom g;
    if (gn_geometry(N, H, W, C, groups, &g) != ISEGMI_OK || groupnorm_is_slab(H, W)) return 0;
    return N * gn_chunks(g) * groups * 16 + N * groups * 16;
}

int groupnorm_launch(const float* x, int64_t N, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, const float* residual,
                     int relu, float* out, void* ws, int64_t ws_bytes, hipStream_t st) {
    GnGeom g;
    TRY(gn_geometry(N, H, W, C, groups, &g));
    if (N == 0) return ISEGMI_OK;
    ARG_CHECK(x && gamma && beta && out, "group_norm: null pointer");
    ARG_CHECK(((uintptr_t)x | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)residual) % 16 == 0, "group_norm: pointers must be 16-byte aligned");
    if (groupnorm_is_slab(H, W)) {
        const int64_t blocks = N * g.ntiles;
        ARG_CHECK(blocks <= 0x7fffffff, "group_norm: too many slabs");
        hipLaunchKernelGGL(gn_slab_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, st, x, g, gamma, beta, eps, residual, relu, out);
        HIP_TRY(hipGetLastError());
        return ISEGMI_OK;
    }
    const int64_t nchunks = gn_chunks(g), blocks = N * nchunks * g.ntiles;
    ARG_CHECK(blocks <= 0x7fffffff && N * groups <= 0x7fffffff, "group_norm: too many blocks");
    ARG_CHECK(ws && ws_bytes >= groupnorm_workspace_bytes(N, H, W, C, groups) && (uintptr_t)ws % 16 == 0, "group_norm: workspace too small (groupnorm_workspace_bytes)");
    double* part = (double*)ws;
    float* stat = (float*)(part + N * nchunks * groups * 2);
    hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, st, x, g, (int)nchunks, part);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)(N * groups)), dim3(64), 0, st, x, g, (int)nchunks, part, eps, stat);
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, st, x, g, (int)nchunks, stat, gamma, beta, residual, relu, out);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi
