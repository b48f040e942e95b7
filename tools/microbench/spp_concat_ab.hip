// spp_concat_ab.hip -- stand-alone A/B of spp_concat_kernel's block size and slab width (csrc/yolo_pool.hip): the kernel with the thread count as a
// template argument and the slab width as an argument; every form is compared bit for bit with the first, then timed over 1000 back-to-back launches between
// HIP events, in two rounds.  Record: profiles/spp_concat_slab_ab.txt.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o spp_concat_ab spp_concat_ab.hip && ./spp_concat_ab
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
constexpr int SPP_PLANE = 8192;
__device__ __forceinline__ void fold4(float4& m, const float4 v) {
    m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
}
template <int NT>
__global__ __launch_bounds__(NT) void spp_kernel(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4, int s4_log2, int zero_pad) {
    __shared__ float4 a[SPP_PLANE / 4];
    __shared__ float4 t[SPP_PLANE / 4];
    const int S4 = 1 << s4_log2, slabs = C4 >> s4_log2;
    const int n = (int)blockIdx.x / slabs, slab = (int)blockIdx.x - n * slabs;
    const int np = H * W, ne = np << s4_log2;
    const float4* src = in + (int64_t)n * np * C4 + slab * S4;
    float4* dst = out + (int64_t)n * np * 4 * C4 + slab * S4;
    for (int i = threadIdx.x; i < ne; i += NT) {
        const int pix = i >> s4_log2, q = i & (S4 - 1);
        const float4 v = src[(int64_t)pix * C4 + q];
        a[i] = v;
        dst[(int64_t)pix * 4 * C4 + 3 * C4 + q] = v;
    }
    __syncthreads();
    const int rs = W << s4_log2;
#pragma unroll 1
    for (int stage = 0; stage < 3; ++stage) {
        for (int i = threadIdx.x; i < ne; i += NT) {
            const int pix = i >> s4_log2;
            const int x = pix % W;
            float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if ((unsigned)(x + d) < (unsigned)W) fold4(m, a[i + d * S4]);
            t[i] = m;
        }
        __syncthreads();
        const int r = 2 * stage + 2;
        for (int i = threadIdx.x; i < ne; i += NT) {
            const int pix = i >> s4_log2, q = i & (S4 - 1);
            const int y = pix / W, x = pix - y * W;
            float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if ((unsigned)(y + d) < (unsigned)H) fold4(m, t[i + d * rs]);
            a[i] = m;
            if (zero_pad && (x < r || y < r || x + r >= W || y + r >= H)) fold4(m, make_float4(0.f, 0.f, 0.f, 0.f));
            dst[(int64_t)pix * 4 * C4 + (2 - stage) * C4 + q] = m;
        }
        __syncthreads();
    }
}
static void launch(int nt, const float* in, float* out, int N, int H, int W, int C, int s4, hipStream_t st) {
    const unsigned blocks = (unsigned)(N * ((C / 4) >> s4));
    if (nt == 256) hipLaunchKernelGGL(spp_kernel<256>, dim3(blocks), dim3(256), 0, st, (const float4*)in, (float4*)out, H, W, C / 4, s4, 0);
    else if (nt == 512) hipLaunchKernelGGL(spp_kernel<512>, dim3(blocks), dim3(512), 0, st, (const float4*)in, (float4*)out, H, W, C / 4, s4, 0);
    else hipLaunchKernelGGL(spp_kernel<1024>, dim3(blocks), dim3(1024), 0, st, (const float4*)in, (float4*)out, H, W, C / 4, s4, 0);
}
int main() {
    const int C = 512;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int sides[2] = {13, 19}, batches[2] = {1, 8}, nts[3] = {256, 512, 1024};
    for (int si = 0; si < 2; ++si) for (int bi = 0; bi < 2; ++bi) {
        const int S = sides[si], N = batches[bi];
        const size_t ne = (size_t)N * S * S * C;
        std::vector<float> h(ne);
        srand(7);
        for (auto& v : h) v = (float)((double)rand() / RAND_MAX - 0.5);
        float *din, *dout, *dref;
        CK(hipMalloc(&din, ne * 4)); CK(hipMalloc(&dout, ne * 16)); CK(hipMalloc(&dref, ne * 16));
        CK(hipMemcpy(din, h.data(), ne * 4, hipMemcpyHostToDevice));
        int s4max = 3;
        while ((S * S * 4) << s4max > SPP_PLANE) --s4max;
        launch(256, din, dref, N, S, S, C, s4max, nullptr);
        CK(hipDeviceSynchronize());
        std::vector<float> ref(ne * 4), got(ne * 4);
        CK(hipMemcpy(ref.data(), dref, ne * 16, hipMemcpyDeviceToHost));
        for (int round = 0; round < 2; ++round)   // two rounds over all forms: the spread
        for (int s4 = s4max; s4 >= 1; --s4) for (int ni = 0; ni < 3; ++ni) {
            const int nt = nts[ni];
            CK(hipMemset(dout, 0xff, ne * 16));
            launch(nt, din, dout, N, S, S, C, s4, nullptr);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(got.data(), dout, ne * 16, hipMemcpyDeviceToHost));
            const bool same = memcmp(got.data(), ref.data(), ne * 16) == 0;
            for (int w = 0; w < 20; ++w) launch(nt, din, dout, N, S, S, C, s4, nullptr);
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0, nullptr));
            for (int r = 0; r < 1000; ++r) launch(nt, din, dout, N, S, S, C, s4, nullptr);
            CK(hipEventRecord(e1, nullptr)); CK(hipEventSynchronize(e1));
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            printf("map %dx%d bs %d  slab %2d ch  threads %4d  blocks %4d  %.2f us  same=%d  round %d\n", S, S, N, 4 << s4, nt, N * ((C / 4) >> s4), ms, (int)same, round);
            if (!same) return 2;
        }
        CK(hipFree(din)); CK(hipFree(dout)); CK(hipFree(dref));
    }
    return 0;
}
