// resample.hip -- PIL-exact 8-bit bilinear resampling on the device: the resize the R-CNN front ends and the YOLOv3
// letterbox did on the host with PIL, fused with what the host paths do behind it (mean / std / channel swap / padding), one launch per batch.
//
// The contract is PIL's Resample.c at 8 bits per channel:
//   tables (host, double, no contraction; isegmi_resample_coeffs): per output index xx of an axis I -> O
//       scale = I / O, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1, center = (xx + 0.5) scale,
//       xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), I) - xmin,
//       w[x] = tri((x + xmin - center + 0.5) / fs) normalised by their sum in index order, k[x] = (int)(w[x] 2^22 + 0.5), unused slots 0
//   pixel: clip8((2^21 + sum_x p[xmin + x] k[x]) >> 22) in int32; the horizontal pass first, ROUNDED TO BYTES, then the vertical pass over those bytes.
// Integer arithmetic only: the result is bit-identical to PIL for any tables the builder makes, and an axis with I == O comes out as an exact copy
// (its tables are one tap of 2^22), so the kernel has no identity branch.
//
// One workgroup (192 threads) owns a kTileH x kTileW tile of the output canvas.  It streams the source rows the tile needs through LDS in chunks of
// kChunkRows: the horizontal pass writes a chunk's rows, already reduced to the tile's kTileW columns, as BYTES (kChunkRows x kTileW x 3 = 6 KB, whatever
// the scale), the vertical pass adds the chunk's share to int32 accumulators in registers -- a thread owns one dword (4 consecutive bytes) of the tile's
// 192-byte row in 4 of its 16 rows, so one LDS read feeds four multiply-adds.  The intermediate image never exists in HBM.  Source bytes are read with
// byte loads (rows start at any address: Win * 3 is odd and images are packed back to back), so there is no alignment case to get wrong.
// No atomics, no cross-block traffic: every output element is written exactly once by one thread.
#include "../../include/isegmi.h"
#include "common.h"

namespace isegmi {

constexpr int kTileH = 16, kTileW = 64, kChunkRows = 32;
constexpr int kRowBytes = kTileW * 3, kRowDwords = kRowBytes / 4;   // 192 B, 48 dwords
constexpr int kThreads = kRowDwords * 4;                            // 192: 4 row groups of 48 dword owners
constexpr int kRowsPerThread = kTileH / 4;
constexpr int kWords = ISEGMI_RESAMPLE_ENTRY_WORDS;

// One image of the batch, as the table row holds it (include/isegmi.h lists the words)
struct RsEntry {
    int64_t src_off, out_off;
    int Hin, Win, Hout, Wout, dst_y, dst_x, ch, cv, ksh, ksv, hflip, plane;
};
__host__ __device__ inline RsEntry rs_entry(const int32_t* w) {
    RsEntry e;
    e.src_off = (int64_t)(uint32_t)w[0] | ((int64_t)w[1] << 32);
    e.Hin = w[2]; e.Win = w[3]; e.Hout = w[4]; e.Wout = w[5]; e.dst_y = w[6]; e.dst_x = w[7];
    e.ch = w[8]; e.cv = w[9]; e.ksh = w[10]; e.ksv = w[11]; e.hflip = w[12]; e.plane = w[13];
    e.out_off = (int64_t)(uint32_t)w[14] | ((int64_t)w[15] << 32);
    return e;
}

struct RsArgs {
    const uint8_t* src;
    const int32_t* table;
    const int32_t* coeffs;
    float* out_f32;      // epilogue (b): fp32 NHWC3 canvas planes; nullptr: epilogue (a), bytes
    uint8_t* out_u8;
    int Hpad, Wpad, swap;
    int64_t out_img_stride;   // floats
    float mean[3], stdv[3], fill;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ void __launch_bounds__(kThreads) resample_u8_kernel(const RsArgs a) {
    __shared__ uint32_t lds[kChunkRows * kRowDwords];
    uint8_t* ldsb = (uint8_t*)lds;
    const RsEntry e = rs_entry(a.table + (int64_t)blockIdx.z * kWords);
    const bool f32 = a.out_f32 != nullptr;
    // the canvas this image is written on: the shared padded canvas (b), or the image itself (a)
    const int Hc = f32 ? a.Hpad : e.Hout, Wc = f32 ? a.Wpad : e.Wout;
    const int dy = f32 ? e.dst_y : 0, dx = f32 ? e.dst_x : 0;
    const int Y0 = blockIdx.y * kTileH, X0 = blockIdx.x * kTileW;
    if (Y0 >= Hc || X0 >= Wc) return;   // (a): the grid is sized for the largest image of the batch
    const int tid = threadIdx.x;
    const int dw = tid % kRowDwords, rg = tid / kRowDwords;

    // image rows / columns of this tile: y in [ya, yb), tile-local px in [pa, pb)
    const int ya = max(Y0 - dy, 0), yb = min(Y0 + kTileH - dy, e.Hout);
    const int pa = max(dx - X0, 0), pb = min(dx + e.Wout - X0, kTileW);
    const bool any = ya < yb && pa < pb;

    int acc[kRowsPerThread][4];
    int vmin[kRowsPerThread], vn[kRowsPerThread];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 1 << 21;
        vmin[i] = 0; vn[i] = 0;
    }
    if (any) {
        const int32_t* bv = a.coeffs + e.cv;                    // [Hout][2]
        const int32_t* kv = bv + 2 * (int64_t)e.Hout;           // [Hout][ksv]
        const int32_t* bh = a.coeffs + e.ch;                    // [Wout][2]
        const int32_t* kh = bh + 2 * (int64_t)e.Wout;           // [Wout][ksh]
        const uint8_t* img = a.src + e.src_off;
        // bounds are clamped to the image: tables from anywhere but the builder cannot make the kernel read outside its source
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int y = Y0 + rg + 4 * i - dy;
            if (y >= ya && y < yb) {
                const int m = min(max(bv[2 * y], 0), e.Hin - 1);
                vmin[i] = m;
                vn[i] = max(min(min(bv[2 * y + 1], e.ksv), e.Hin - m), 0);
            }
        }
        const int lo = min(max(bv[2 * ya], 0), e.Hin - 1);
        const int mlast = min(max(bv[2 * (yb - 1)], 0), e.Hin - 1);
        const int hi = mlast + max(min(min(bv[2 * (yb - 1) + 1], e.ksv), e.Hin - mlast), 0);
        for (int r0 = lo; r0 < hi; r0 += kChunkRows) {
            const int rows = min(kChunkRows, hi - r0);
            // horizontal pass: source rows r0 .. r0 + rows, the tile's columns, rounded to bytes
            const int ncol = pb - pa;
            for (int it = tid; it < rows * ncol; it += kThreads) {
                const int r = it / ncol, px = pa + it - r * ncol;
                const int x = X0 + px - dx;
                const int rc = e.hflip ? e.Wout - 1 - x : x;    // the mirror of the RESIZED image: output column x shows resized column Wout - 1 - x
                const int xm = min(max(bh[2 * rc], 0), e.Win - 1);
                const int n = max(min(min(bh[2 * rc + 1], e.ksh), e.Win - xm), 0);
                const int32_t* k = kh + (int64_t)rc * e.ksh;
                const uint8_t* p = img + ((int64_t)(r0 + r) * e.Win + xm) * 3;
                int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
                for (int j = 0; j < n; ++j) {
                    const int kj = k[j];
                    s0 += (int)p[3 * j] * kj; s1 += (int)p[3 * j + 1] * kj; s2 += (int)p[3 * j + 2] * kj;
                }
                uint8_t* o = ldsb + r * kRowBytes + px * 3;
                o[0] = (uint8_t)clip8(s0 >> 22); o[1] = (uint8_t)clip8(s1 >> 22); o[2] = (uint8_t)clip8(s2 >> 22);
            }
            __syncthreads();
            // vertical pass: this chunk's share of every owned output row
#pragma unroll
            for (int i = 0; i < kRowsPerThread; ++i) {
                const int s_lo = max(vmin[i], r0), s_hi = min(vmin[i] + vn[i], r0 + rows);
                if (s_lo < s_hi) {
                    const int y = Y0 + rg + 4 * i - dy;
                    const int32_t* k = kv + (int64_t)y * e.ksv;
                    for (int s = s_lo; s < s_hi; ++s) {
                        const uint32_t v = lds[(s - r0) * kRowDwords + dw];
                        const int ks = k[s - vmin[i]];
                        acc[i][0] += (int)(v & 255u) * ks; acc[i][1] += (int)((v >> 8) & 255u) * ks;
                        acc[i][2] += (int)((v >> 16) & 255u) * ks; acc[i][3] += (int)(v >> 24) * ks;
                    }
                }
            }
            __syncthreads();
        }
    }
    // epilogue: every canvas element of the tile is written exactly once
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        const int Y = Y0 + rg + 4 * i;
        if (Y >= Hc) continue;
        const bool row_in = any && Y - dy >= ya && Y - dy < yb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = dw * 4 + j, px = b / 3, c = b - px * 3;
            const int X = X0 + px;
            if (X >= Wc) continue;
            const bool in = row_in && px >= pa && px < pb;
            if (f32) {
                float* o = a.out_f32 + (int64_t)e.plane * a.out_img_stride + ((int64_t)Y * Wc + X) * 3;
                if (in) o[a.swap ? 2 - c : c] = ((float)clip8(acc[i][j] >> 22) - a.mean[c]) / a.stdv[c];
                else o[c] = a.fill;
            } else if (in) {
                a.out_u8[e.out_off + ((int64_t)Y * Wc + X) * 3 + c] = (uint8_t)clip8(acc[i][j] >> 22);
            }
        }
    }
}

// PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, host only.  This file is compiled with -ffp-contract=off: every product
// and sum below is rounded on its own, as in PIL's C.
static inline double tri(double t) {
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}
static int resample_ksize(int I, int O) {
    double fs = (double)I / (double)O;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(fs) * 2 + 1;
}

int resample_u8_launch(const uint8_t* d_src, int64_t src_bytes, const int32_t* d_table, const int32_t* h_table, int N, const int32_t* d_coeffs,
                       int64_t coeff_words, float* d_out, int planes, int Hpad, int Wpad, int64_t out_img_stride, const float* mean3, const float* std3,
                       int swap_rb, float fill, uint8_t* d_out_u8, int64_t out_u8_bytes, hipStream_t st) {
    ARG_CHECK(d_src && d_table && h_table && d_coeffs && N > 0 && N <= 65535, "resample_u8 args (the host copy of the table is required: it is validated here)");
    ARG_CHECK((d_out != nullptr) != (d_out_u8 != nullptr), "resample_u8: exactly one of the fp32 canvas and the byte output");
    int gh = 0, gw = 0;
    if (d_out) {
        ARG_CHECK(mean3 && std3 && planes > 0 && Hpad > 0 && Wpad > 0 && out_img_stride >= (int64_t)Hpad * Wpad * 3, "resample_u8 canvas");
        gh = Hpad; gw = Wpad;
    }
    for (int i = 0; i < N; ++i) {
        const RsEntry e = rs_entry(h_table + (int64_t)i * kWords);
        ARG_CHECK(e.Hin > 0 && e.Win > 0 && e.Hout > 0 && e.Wout > 0, "resample_u8 table: image sizes");
        ARG_CHECK(e.src_off >= 0 && e.src_off + (int64_t)e.Hin * e.Win * 3 <= src_bytes, "resample_u8 table: source bytes outside the source buffer");
        ARG_CHECK(e.ksh == resample_ksize(e.Win, e.Wout) && e.ksv == resample_ksize(e.Hin, e.Hout) && e.ksh <= ISEGMI_RESAMPLE_MAX_KSIZE &&
                  e.ksv <= ISEGMI_RESAMPLE_MAX_KSIZE, "resample_u8 table: ksize (at most ISEGMI_RESAMPLE_MAX_KSIZE = 1025 taps per axis)");
        ARG_CHECK(e.ch >= 0 && (int64_t)e.ch + (int64_t)e.Wout * (2 + e.ksh) <= coeff_words && e.cv >= 0 &&
                  (int64_t)e.cv + (int64_t)e.Hout * (2 + e.ksv) <= coeff_words, "resample_u8 table: coefficient tables outside the coefficient buffer");
        if (d_out) {
            ARG_CHECK(e.dst_y >= 0 && e.dst_x >= 0 && e.dst_y + e.Hout <= Hpad && e.dst_x + e.Wout <= Wpad && e.plane >= 0 && e.plane < planes,
                      "resample_u8 table: image outside the canvas");
        } else {
            ARG_CHECK(e.out_off >= 0 && e.out_off + (int64_t)e.Hout * e.Wout * 3 <= out_u8_bytes, "resample_u8 table: output bytes outside the output buffer");
            gh = e.Hout > gh ? e.Hout : gh; gw = e.Wout > gw ? e.Wout : gw;
        }
    }
    const int gy = cdiv(gh, kTileH);
    ARG_CHECK(gy <= 65535, "resample_u8: more than 65535 tile rows");
    RsArgs a;
    a.src = d_src; a.table = d_table; a.coeffs = d_coeffs; a.out_f32 = d_out; a.out_u8 = d_out_u8;
    a.Hpad = Hpad; a.Wpad = Wpad; a.swap = swap_rb ? 1 : 0; a.out_img_stride = out_img_stride; a.fill = fill;
    for (int c = 0; c < 3; ++c) { a.mean[c] = d_out ? mean3[c] : 0.0f; a.stdv[c] = d_out ? std3[c] : 1.0f; }
    hipLaunchKernelGGL(resample_u8_kernel, dim3(cdiv(gw, kTileW), gy, N), dim3(kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return ISEGMI_OK;
}

}  // namespace isegmi

using namespace isegmi;

extern "C" int isegmi_resample_coeffs(int I, int O, int32_t* bounds, int32_t* kk, int* ksize) {
    ARG_CHECK(I >= 1 && O >= 1, "resample_coeffs: I, O >= 1");
    ARG_CHECK(ksize, "null");
    const double scale = (double)I / (double)O;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    ARG_CHECK(ceil(support) <= (double)((ISEGMI_RESAMPLE_MAX_KSIZE - 1) / 2),
              "resample_coeffs: the scale I / O is beyond the cap ISEGMI_RESAMPLE_MAX_KSIZE (ksize = 2 ceil(I / O) + 1 <= 1025)");
    const int ks = (int)ceil(support) * 2 + 1;
    *ksize = ks;
    if (!bounds && !kk) return ISEGMI_OK;   // the size query
    ARG_CHECK(bounds && kk, "resample_coeffs: both tables or neither");
    const double ss = 1.0 / fs;
    double w[ISEGMI_RESAMPLE_MAX_KSIZE];
    for (int xx = 0; xx < O; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > I) xmax = I;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = tri((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = kk + (int64_t)xx * ks;
        for (int x = 0; x < ks; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0.0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ISEGMI_OK;
}

extern "C" int isegmi_op_resample_tile(int* tile_h, int* tile_w, int* chunk_rows) {
    ARG_CHECK(tile_h && tile_w && chunk_rows, "null");
    *tile_h = kTileH; *tile_w = kTileW; *chunk_rows = kChunkRows;
    return ISEGMI_OK;
}

extern "C" int isegmi_op_resample_u8(const uint8_t* d_src, int64_t src_bytes, const int32_t* d_table, const int32_t* h_table, int N,
                                     const int32_t* d_coeffs, int64_t coeff_words, float* d_out, int planes, int Hpad, int Wpad, int64_t out_img_stride,
                                     const float* mean3, const float* std3, int swap_rb, float fill, uint8_t* d_out_u8, int64_t out_u8_bytes,
                                     void* stream) {
    return resample_u8_launch(d_src, src_bytes, d_table, h_table, N, d_coeffs, coeff_words, d_out, planes, Hpad, Wpad, out_img_stride, mean3, std3,
                              swap_rb, fill, d_out_u8, out_u8_bytes, (hipStream_t)stream);
}
