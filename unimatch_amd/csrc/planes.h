// fp32 -> 16-bit operand planes (the MFMA operand format of the attention / correlation kernels).
//   exact mode: 2 planes of fp16,  x*scale = hi + lo  (hi = rn16(x*scale), lo = rn16(x*scale - hi))
//   fast  mode: 1 plane of bf16
// Plane layout: [NS][rows][128] 16-bit, plane stride = rows*128 elements.
#pragma once
#include "common.h"
#include "timing.h"

template <class T, int NS>
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ src,
                                                           unsigned short* __restrict__ dst,
                                                           long n8, float scale, long plane_stride, unsigned* range_flag) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long step = (long)gridDim.x * blockDim.x;
    float mx = 0.f;
    for (; i < n8; i += step) {
        const f32x4* s4 = reinterpret_cast<const f32x4*>(src) + 2 * i;
        f32x4 a = s4[0], b = s4[1];
        float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        float y[8];
        u32x4 hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            y[j] = x[j] * scale;
            mx = fmaxf(mx, __builtin_fabsf(y[j]));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) hi[j] = T::pack2(y[2 * j], y[2 * j + 1]);
        *reinterpret_cast<u32x4*>(dst + 8 * i) = hi;
        if (NS == 2) {
            u32x4 lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x2 h = T::unpack2(hi[j]);
                lo[j] = T::pack2(y[2 * j] - h[0], y[2 * j + 1] - h[1]);
            }
            *reinterpret_cast<u32x4*>(dst + plane_stride + 8 * i) = lo;
        }
    }
    um_range_note<T>(range_flag, mx, UM_RANGE_PLANES);
}

// ---- the value a normalisation pass writes, 8 channels of one pixel at a time -- ONE function for nhwc_apply_kernel (nhwc_ops.hip)
// and for the convolution that builds the same operand while it stages it (conv_kernel's entry variant, conv.hip), so that the two
// cannot drift: same operations, same order, no contraction (every product and sum is rounded on its own).
//   v = (v - mu) * rs              if norm
//   v = max(v, 0)                  if relu
//   v = max(v + s, 0)              sc == 1: s = fp32 shortcut, itself (s - smu) * srs first when sc_norm (a projection shortcut's own
//                                  InstanceNorm, computed here instead of in a pass of its own)
//   v = max(v + (s_hi + s_lo), 0)  sc == 2: shortcut as operand planes
//   h = pack(v), l = pack(v - unpack(h))                                          if split
template <class T, int NS>
__device__ __forceinline__ void um_norm_value8(float (&v)[8], bool norm, const float (&mu)[8], const float (&rs)[8], bool relu, int sc,
                                               float (&s)[8], bool sc_norm, const float (&smu)[8], const float (&srs)[8], u32x4 sh,
                                               u32x4 sl, bool split, u32x4& h, u32x4& l) {
#pragma clang fp contract(off)
    if (norm) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (v[i] - mu[i]) * rs[i];
    }
    if (relu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
    }
    if (sc == 1) {
        if (sc_norm) {
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = (s[i] - smu[i]) * srs[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i] + s[i], 0.f);
    } else if (sc == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 uh = T::unpack2(sh[i]);
            f32x2 ul = {0.f, 0.f};
            if (NS == 2) ul = T::unpack2(sl[i]);
            v[2 * i] = fmaxf(v[2 * i] + (uh[0] + ul[0]), 0.f);
            v[2 * i + 1] = fmaxf(v[2 * i + 1] + (uh[1] + ul[1]), 0.f);
        }
    }
    if (split) {
        h = u32x4{T::pack2(v[0], v[1]), T::pack2(v[2], v[3]), T::pack2(v[4], v[5]), T::pack2(v[6], v[7])};
        if (NS == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x2 u = T::unpack2(h[i]);
                l[i] = T::pack2(v[2 * i] - u[0], v[2 * i + 1] - u[1]);
            }
        }
    }
}

// n_elems fp32 values (a multiple of 8) -> planes at dst, plane stride n_elems.  Returns hipError_t of the launch.
static inline hipError_t launch_split_elems(const float* src, unsigned short* dst, long n_elems, float scale,
                                            int mode, hipStream_t stream);

// rows*128 fp32 values -> planes at dst.
static inline hipError_t launch_split_planes(const float* src, unsigned short* dst, long rows, float scale,
                                             int mode, hipStream_t stream) {
    return launch_split_elems(src, dst, rows * UM_CHANNELS, scale, mode, stream);
}

static inline hipError_t launch_split_elems(const float* src, unsigned short* dst, long n_elems, float scale,
                                            int mode, hipStream_t stream) {
    const long n8 = n_elems / 8;
    long blocks = (n8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    const long plane_stride = n_elems;
    ScopedKernelTimer timer(UM_K_SPLIT_PLANES, stream);
    if (mode == 0)
        hipLaunchKernelGGL((split_planes_kernel<Fp16, 2>), dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, n8,
                           scale, plane_stride, um_range_flag_dev());
    else
        hipLaunchKernelGGL((split_planes_kernel<Bf16, 1>), dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, n8,
                           scale, plane_stride, (unsigned*)nullptr);
    return hipGetLastError();
}

static inline size_t planes_bytes(long rows, int mode) {
    return (size_t)rows * UM_CHANNELS * 2 * (mode == 0 ? 2 : 1);
}
