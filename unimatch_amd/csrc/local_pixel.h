// Per-pixel pieces of the local-window kernels (local_ops.hip) that the multi-view plane sweep (depth_multi.hip) shares: the
// 128-channel row split over the 4 lanes of a tap slot, the slot reductions, and the statistics record of the plane sweep (K7).
// Everything here is __forceinline__ device code, moved out of local_ops.hip unchanged: that file's kernels compile as before.
#pragma once
#include "common.h"

#define LOCAL_MAX_ROUNDS 8      // up to 128 taps / depth candidates

// A 128-channel fp32 row (512 B) is shared by the 4 lanes of a tap slot.  Lane quarter q owns channels 16 i + 4 q .. + 3
// (i = 0..7): callers pass `row + 4 * quarter`, and load i of the four lanes covers 64 CONTIGUOUS bytes -- one request to
// the L1 per slot and load.  (Round 1 gave each lane 32 consecutive channels: four 16-byte pieces 128 B apart per slot and
// load, i.e. 64 cache lines touched by every wave instruction; these gather kernels were bound by exactly that.)
__device__ __forceinline__ void load32(f32x4 (&r)[8], const float* p) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = reinterpret_cast<const f32x4*>(p)[4 * i];
}

__device__ __forceinline__ float dot32(const f32x4 (&a)[8], const float* p) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4 b = reinterpret_cast<const f32x4*>(p)[4 * i];
        acc = __builtin_fmaf(a[i][0], b[0], acc);
        acc = __builtin_fmaf(a[i][1], b[1], acc);
        acc = __builtin_fmaf(a[i][2], b[2], acc);
        acc = __builtin_fmaf(a[i][3], b[3], acc);
    }
    return acc;
}

__device__ __forceinline__ float quad_sum(float v) {      // sum over the 4 channel quarters (lanes 4k..4k+3)
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}
__device__ __forceinline__ float slot_max(float v) {      // reduce over the 16 tap slots (lane bits 2..5)
    v = fmaxf(v, __shfl_xor(v, 4));
    v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}
__device__ __forceinline__ float slot_sum(float v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// ---- K7, the plane sweep: what one pixel yields next to its prediction (see depth_pixel_gather in local_ops.hip) -----------------
struct DepthPixelStats {
    float max_prob, entropy, variance, peak_mass;
    int best, in_view;
};

// ln of the softmax denominator (1 <= v <= 128), once per pixel.  v = m 2^k with m in [0.75, 1.5): k ln 2 carries the size and is
// formed in two pieces (k * hi is exact: hi has 16 significant bits), logf(m) is small, so its error is a fraction of an ulp of the
// result.  A uniform distribution (sum e = D exactly, every other term of the entropy 0) then gives ln D to within one ulp; logf(v)
// alone is 1.06 ulp off at D = 17, and a log through fp64 costs the box kernel a wave of occupancy (173 VGPRs).
__device__ __forceinline__ float depth_ln(float v) {
    int k;
    float m = frexpf(v, &k);                                   // m in [0.5, 1)
    if (m < 0.75f) { m *= 2.f; k -= 1; }
    const float kf = (float)k;
    return __builtin_fmaf(kf, 0.693145751953125f, __builtin_fmaf(kf, 1.428606765330187e-06f, logf(m)));
}

__device__ __forceinline__ int slot_sum_i(int v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int slot_min_i(int v) {
    v = min(v, __shfl_xor(v, 4));
    v = min(v, __shfl_xor(v, 8));
    v = min(v, __shfl_xor(v, 16));
    v = min(v, __shfl_xor(v, 32));
    return v;
}

// lane 0 of the pixel's wave writes the statistics planes (stats [B, 4, h, w], index [B, 2, h, w]; either may be null)
__device__ __forceinline__ void depth_stats_store(float* __restrict__ stats, int* __restrict__ index, int b, int p, int L,
                                                  const DepthPixelStats& st) {
    if (stats) {
        float* sp = stats + (long)b * 4 * L + p;
        sp[0] = st.max_prob;
        sp[L] = st.entropy;
        sp[2 * (long)L] = st.variance;
        sp[3 * (long)L] = st.peak_mass;
    }
    if (index) {
        int* ip = index + (long)b * 2 * L + p;
        ip[0] = st.best;
        ip[L] = st.in_view;
    }
}

// rows of the wave-private table of the box form (depth_corr_softmax_box_body): a larger bounding box takes the gather form
#define DEPTH_BOX 160

// one wave per pixel, four per workgroup
static inline unsigned pixel_grid_blocks(long pixels) {
    long blocks = (pixels + 3) / 4;
    const long cap = 256 * 16;           // 16 workgroups per CU, grid-stride beyond
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}
