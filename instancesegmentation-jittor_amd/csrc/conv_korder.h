// conv_korder.h -- the K order of the fp32 convolutions, in ONE place: what isegmi_pack_conv_weights writes, what the MFMA kernels of conv_mfma.hip walk,
// and what any other kernel must walk to reproduce a convolution output bit for bit (yolact_coeff.hip).
//
// A packed weight row holds the R*S*Cin products' weights in (r, s, cin) order, in 32-float CHUNKS; inside each group of 8 consecutive k the floats
// sit as [k0 k2 k4 k6 | k1 k3 k5 k7] (conv_perm8).  The accumulator chain of one output walks: channel groups of `kgroup` chunks outermost
// (conv_kgroup: 128 channels for a spatial kernel, all of Cin for a 1x1), then the taps (r, s), then the group's chunks, k ascending inside a chunk.
#pragma once

namespace isegmi {

constexpr int CONV_KGROUP_CHUNKS = 4;  // 128 input channels per K group (ORA_CONV_CGROUP in the oracle)

// position of k (0..7 within its 8-group) in the packed row
__host__ __device__ inline int conv_perm8(int e) { return 4 * (e & 1) + (e >> 1); }

// chunks per channel group of a layer with cin_chunks = Cin / 32 (the stem is one group)
__host__ __device__ inline int conv_kgroup(int R, int S, int cin_chunks, bool stem) {
    return (R * S == 1 || stem) ? cin_chunks : (cin_chunks < CONV_KGROUP_CHUNKS ? cin_chunks : CONV_KGROUP_CHUNKS);
}

// chunk index inside the packed weight row of walk position (tap (kr, ks), chunk kc of the channel group that starts at chunk kg)
__host__ __device__ __forceinline__ int conv_k_wchunk(int kr, int ks, int kc, int kg, int S, int cin_chunks) { return (kr * S + ks) * cin_chunks + kg + kc; }

// One step of the walk: (kr, ks, kc, kg, glen) -> the next chunk's position; glen = chunks of the current channel group (kgroup to start with).  True when
// the TAP changed (the next chunk reads another input pixel, or the first tap again for the next channel group).  Past the last chunk the position wraps
// to a harmless one (the kernels' loads there are dead).
__host__ __device__ __forceinline__ bool conv_k_next(int& kr, int& ks, int& kc, int& kg, int& glen, int R, int S, int kgroup, int cin_chunks) {
    if (++kc != glen) return false;
    kc = 0;
    if (++ks == S) {
        ks = 0;
        if (++kr == R) { kr = 0; kg += glen; glen = kgroup < cin_chunks - kg ? kgroup : cin_chunks - kg; if (glen <= 0) { glen = 1; kg = 0; } }
    }
    return true;
}

}  // namespace isegmi
