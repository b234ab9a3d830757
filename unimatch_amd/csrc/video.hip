// Video post-processing: forward-backward occlusion masks, Middlebury flow colouring and point tracks.       gfx950 / wave64
//
// All are memory-bound, one thread per pixel (or four, or per track), and none keeps any state between calls:
//
//   um_fwd_bwd_occlusion  forward_backward_consistency_check (unimatch/geometry.py:75-96) in ONE launch: the reference runs two
//                         grid_sample warps and about a dozen element-wise ATen kernels.  Per pixel and direction: bilinear sample
//                         of the other flow at p + flow(p) (zeros outside, align_corners), |flow + warped| > alpha (|fwd| + |bwd|) + beta.
//   um_flow_to_rgb        flow_to_image (utils/flow_viz.py:231-254 with compute_color :185-228) per image of a batch, on the device:
//                         the reference copies 8 B/px to the host and runs float64 NumPy.  Two deterministic launches:
//                         flow_rgb_max_kernel writes one partial maximum radius per workgroup into the workspace (every slot of the
//                         launch's geometry is rewritten each call: nothing from an earlier call is ever read), flow_rgb_kernel folds
//                         its image's partials and colours.  No atomics, no arrival counters.
//   um_flow_chain         follows points through the P flows of a sequence in ONE launch: a thread owns a track and keeps its position
//                         and alive flag in registers over the P steps, so the state never goes through HBM between steps (a loop of
//                         torch ops is about a dozen launches per step, each moving the whole state).  No reference code: the step is
//                         the composition F(0->t+1) = F(0->t) + flow_warp(F(t->t+1), F(0->t)) of unimatch/geometry.py's flow_warp.
//
// Rounding follows the reference step by step (NumPy 2 promotion rules): |flow| of the colouring is a float32 square root (rounded
// once, __fsqrt_rn); the division by (maxrad + float64 eps) and everything after it -- arctan2, the wheel interpolation, floor -- is
// float64.  The file is compiled with -ffp-contract=off (build.py): a fused multiply-add would round differently from the reference's
// separate products and sums.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

// ---- occlusion ------------------------------------------------------------------------------------------------------------------

// grid_sample(align_corners=True, zeros) of the two channel planes c0 / c1 ([h][w]) at pixel (x, y) + (dx, dy), with the reference's
// coordinate round trip: normalise 2 p / (w - 1) - 1 (geometry.py:52-53), un-normalise ((g + 1) / 2) (w - 1) inside grid_sample.
__device__ __forceinline__ void occ_sample(const float* __restrict__ c0, const float* __restrict__ c1, int h, int w, int x, int y,
                                           float dx, float dy, float& s0, float& s1) {
    const float px = (float)x + dx, py = (float)y + dy;
    const float gx = 2.0f * px / (float)(w - 1) - 1.0f, gy = 2.0f * py / (float)(h - 1) - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(w - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(h - 1);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    const float wnw = (fx1 - ix) * (fy1 - iy), wne = (ix - fx0) * (fy1 - iy);
    const float wsw = (fx1 - ix) * (iy - fy0), wse = (ix - fx0) * (iy - fy0);
    // clamped before the int conversion: a flow far out of frame (or NaN) must not overflow it; every clamped tap is outside
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f), y0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    float a0 = 0.f, a1 = 0.f;
    auto tap = [&](int yy, int xx, float wt) {       // loads from a clamped address without a branch; only in-frame taps add
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const int q = in ? yy * w + xx : 0;
        const float v0 = c0[q], v1 = c1[q];
        a0 = in ? a0 + v0 * wt : a0;
        a1 = in ? a1 + v1 * wt : a1;
    };
    tap(y0, x0, wnw);
    tap(y0, x0 + 1, wne);
    tap(y0 + 1, x0, wsw);
    tap(y0 + 1, x0 + 1, wse);
    s0 = a0;
    s1 = a1;
}

__global__ __launch_bounds__(256) void fwd_bwd_occ_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd,
                                                          float* __restrict__ occ_fwd, float* __restrict__ occ_bwd, int h, int w,
                                                          float alpha, float beta) {
    const int L = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const int b = blockIdx.y;
    const int y = p / w, x = p - y * w;
    const float* f = fwd + (long)b * 2 * L;
    const float* g = bwd + (long)b * 2 * L;
    const float fu = f[p], fv = f[L + p], bu = g[p], bv = g[L + p];
    float wbu, wbv, wfu, wfv;
    occ_sample(g, g + L, h, w, x, y, fu, fv, wbu, wbv);      // backward flow seen from the forward target
    occ_sample(f, f + L, h, w, x, y, bu, bv, wfu, wfv);      // forward flow seen from the backward target
    const float mag = __fsqrt_rn(fu * fu + fv * fv) + __fsqrt_rn(bu * bu + bv * bv);
    const float thr = alpha * mag + beta;
    const float du = fu + wbu, dv = fv + wbv, eu = bu + wfu, ev = bv + wfv;
    const float dfwd = __fsqrt_rn(du * du + dv * dv), dbwd = __fsqrt_rn(eu * eu + ev * ev);
    occ_fwd[(long)b * L + p] = dfwd > thr ? 1.f : 0.f;
    occ_bwd[(long)b * L + p] = dbwd > thr ? 1.f : 0.f;
}

extern "C" int um_fwd_bwd_occlusion(const float* fwd, const float* bwd, float* occ_fwd, float* occ_bwd, int batch, int h, int w,
                                    float alpha, float beta, void* stream) {
    if (!fwd || !bwd || !occ_fwd || !occ_bwd || batch <= 0 || batch > 65535 || h < 2 || w < 2 || (long)h * w > (1L << 30)) {
        um_set_error("um_fwd_bwd_occlusion: bad argument (batch=%d h=%d w=%d)", batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    const long L = (long)h * w;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    hipLaunchKernelGGL(fwd_bwd_occ_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, fwd,
                       bwd, occ_fwd, occ_bwd, h, w, alpha, beta);
    return (int)hipGetLastError();
}

// ---- flow colouring -------------------------------------------------------------------------------------------------------------

#define UM_RGB_MAX_PX 16                       // pixels per thread of the partial-maximum launch (4096 per workgroup)
#define UM_RGB_PX 4                            // pixels per thread of the colour launch (12 output bytes: three 4-byte stores)
#define UM_RGB_CHUNK (256 * UM_RGB_MAX_PX)
#define UM_UNKNOWN_FLOW 1e7f

// the Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow"): 55 hues in six segments
// RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; a ramp entry of segment length n at step i is floor(255 i / n)
// (stored divided by 255, as compute_color uses them: each entry is the correctly rounded float64 quotient, folded at compile time)
#define W3(r, g, b) {r / 255.0, g / 255.0, b / 255.0}
__constant__ double um_wheel[55][3] = {
    W3(255, 0, 0), W3(255, 17, 0), W3(255, 34, 0), W3(255, 51, 0), W3(255, 68, 0), W3(255, 85, 0),
    W3(255, 102, 0), W3(255, 119, 0), W3(255, 136, 0), W3(255, 153, 0), W3(255, 170, 0), W3(255, 187, 0),
    W3(255, 204, 0), W3(255, 221, 0), W3(255, 238, 0), W3(255, 255, 0), W3(213, 255, 0), W3(170, 255, 0),
    W3(128, 255, 0), W3(85, 255, 0), W3(43, 255, 0), W3(0, 255, 0), W3(0, 255, 63), W3(0, 255, 127),
    W3(0, 255, 191), W3(0, 255, 255), W3(0, 232, 255), W3(0, 209, 255), W3(0, 186, 255), W3(0, 163, 255),
    W3(0, 140, 255), W3(0, 116, 255), W3(0, 93, 255), W3(0, 70, 255), W3(0, 47, 255), W3(0, 24, 255),
    W3(0, 0, 255), W3(19, 0, 255), W3(39, 0, 255), W3(58, 0, 255), W3(78, 0, 255), W3(98, 0, 255),
    W3(117, 0, 255), W3(137, 0, 255), W3(156, 0, 255), W3(176, 0, 255), W3(196, 0, 255), W3(215, 0, 255),
    W3(235, 0, 255), W3(255, 0, 255), W3(255, 0, 213), W3(255, 0, 170), W3(255, 0, 128), W3(255, 0, 85),
    W3(255, 0, 43)};
#undef W3

// float32 |flow| of one pixel after the unknown-flow rule (|u| or |v| > 1e7: both zero; a NaN is not unknown and stays)
__device__ __forceinline__ float rgb_rad(float& u, float& v) {
    if (fabsf(u) > UM_UNKNOWN_FLOW || fabsf(v) > UM_UNKNOWN_FLOW) u = v = 0.f;
    return __fsqrt_rn(u * u + v * v);
}

// NaN-propagating maximum (np.max): a NaN anywhere makes the result NaN
__device__ __forceinline__ float nanmax(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

__device__ __forceinline__ float block_nanmax(float m, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    return m;
}

// phase 1: partial[b][chunk] = np.max of |flow| over 4096 pixels of image b (NaN if any is NaN)
__global__ __launch_bounds__(256) void flow_rgb_max_kernel(const float* __restrict__ flow, float* __restrict__ partial, int L, int chunks) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const float* fu = flow + (long)b * 2 * L;
    const float* fv = fu + L;
    float m = 0.f;                                         // |flow| >= 0: 0 is the identity of the maximum
    const int base = blockIdx.x * UM_RGB_CHUNK + threadIdx.x;
#pragma unroll
    for (int i = 0; i < UM_RGB_MAX_PX; ++i) {
        const int p = base + i * 256;
        if (p < L) {
            float u = fu[p], v = fv[p];
            m = nanmax(m, rgb_rad(u, v));
        }
    }
    m = block_nanmax(m, red);
    if (threadIdx.x == 0) partial[(long)b * chunks + blockIdx.x] = m;
}

// compute_color of one pixel, float64 from the normalised (u, v) on; writes floor(255 col) per channel
__device__ __forceinline__ void rgb_pixel(float uf, float vf, double den, unsigned char* out) {
    const bool unknown = fabsf(uf) > UM_UNKNOWN_FLOW || fabsf(vf) > UM_UNKNOWN_FLOW;
    if (unknown) uf = vf = 0.f;
    double u = (double)uf / den, v = (double)vf / den;
    const bool nan = (u != u) || (v != v);
    if (nan) u = v = 0.0;
    const double rad = __dsqrt_rn(u * u + v * v);
    const double a = atan2(-v, -u) / 3.141592653589793;
    const double fk = (a + 1.0) / 2.0 * 54.0 + 1.0;
    const double fl = floor(fk);
    int k0 = (int)fl;
    int k1 = k0 + 1;
    if (k1 == 56) k1 = 1;
    const double f = fk - fl;
    const bool inside = rad <= 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double col0 = um_wheel[k0 - 1][c], col1 = um_wheel[k1 - 1][c];
        double col = (1.0 - f) * col0 + f * col1;
        col = inside ? 1.0 - rad * (1.0 - col) : col * 0.75;
        // (1 - nanIdx) multiplies in compute_color; the unknown-flow pixels are set to 0 afterwards in flow_to_image
        const double val = floor(255.0 * col * (nan ? 0.0 : 1.0));
        out[c] = unknown ? (unsigned char)0 : (unsigned char)(int)val;
    }
}

// phase 2: fold image b's partials into maxrad (max(-1, np.max(rad)): -1 when that maximum is NaN), colour UM_RGB_PX pixels per thread
__global__ __launch_bounds__(256) void flow_rgb_kernel(const float* __restrict__ flow, const float* __restrict__ partial,
                                                       unsigned char* __restrict__ rgb, int L, int chunks, int vec) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    float m = 0.f;
    for (int i = threadIdx.x; i < chunks; i += 256) m = nanmax(m, partial[(long)b * chunks + i]);
    m = block_nanmax(m, red);
    const double den = (m != m ? -1.0 : (double)m) + 2.220446049250313e-16;      // maxrad + np.finfo(float).eps
    const float* fu = flow + (long)b * 2 * L;
    const float* fv = fu + L;
    unsigned char* ob = rgb + (long)b * L * 3;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * UM_RGB_PX;
    if (p0 >= L) return;
    unsigned char px[UM_RGB_PX * 3];
    if (vec && p0 + UM_RGB_PX <= L) {
        // whole group; vec (host): L % 4 == 0, flow 16-byte and rgb 4-byte aligned, so every image's planes are 16-byte aligned and its
        // bytes start at a multiple of 12
        const f32x4 u4 = *reinterpret_cast<const f32x4*>(fu + p0), v4 = *reinterpret_cast<const f32x4*>(fv + p0);
#pragma unroll
        for (int i = 0; i < UM_RGB_PX; ++i) rgb_pixel(u4[i], v4[i], den, px + 3 * i);
        unsigned* dst = reinterpret_cast<unsigned*>(ob + (long)p0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dst[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
        return;
    }
    for (int i = 0; i < UM_RGB_PX && p0 + i < L; ++i) {
        rgb_pixel(fu[p0 + i], fv[p0 + i], den, px);
        ob[(long)(p0 + i) * 3] = px[0];
        ob[(long)(p0 + i) * 3 + 1] = px[1];
        ob[(long)(p0 + i) * 3 + 2] = px[2];
    }
}

static inline bool rgb_args_ok(int batch, int h, int w) {
    return batch > 0 && batch <= 65535 && h > 0 && w > 0 && (long)h * w <= (1L << 30);
}

extern "C" size_t um_flow_to_rgb_workspace_bytes(int batch, int h, int w) {
    if (!rgb_args_ok(batch, h, w)) return 0;
    const long L = (long)h * w;
    return (size_t)batch * (size_t)((L + UM_RGB_CHUNK - 1) / UM_RGB_CHUNK) * sizeof(float);
}

extern "C" int um_flow_to_rgb(const float* flow, unsigned char* rgb, int batch, int h, int w, void* workspace, size_t ws_bytes,
                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!flow || !rgb || !rgb_args_ok(batch, h, w)) {
        um_set_error("um_flow_to_rgb: bad argument (batch=%d h=%d w=%d)", batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_flow_to_rgb_workspace_bytes(batch, h, w);
    if (!workspace || ws_bytes < need) {
        um_set_error("um_flow_to_rgb: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const int L = h * w;
    const int chunks = (L + UM_RGB_CHUNK - 1) / UM_RGB_CHUNK;
    const int groups = (L + 256 * UM_RGB_PX - 1) / (256 * UM_RGB_PX);
    float* partial = (float*)workspace;
    const int vec = (L % 4 == 0) && ((uintptr_t)flow % 16 == 0) && ((uintptr_t)rgb % 4 == 0);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(flow_rgb_max_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(256), 0, stream, flow, partial, L, chunks);
    hipLaunchKernelGGL(flow_rgb_kernel, dim3((unsigned)groups, (unsigned)batch), dim3(256), 0, stream, flow, (const float*)partial, rgb,
                       L, chunks, vec);
    return (int)hipGetLastError();
}

// ---- point tracks ---------------------------------------------------------------------------------------------------------------

// Bilinear sample of the flow planes c0 / c1 (and of the mask plane m, when there is one) at the pixel position (px, py): zeros
// outside, the weights and the tap rule of occ_sample without its normalise / un-normalise round trip.
__device__ __forceinline__ void chain_sample(const float* __restrict__ c0, const float* __restrict__ c1, const float* __restrict__ m,
                                             int h, int w, float px, float py, float& s0, float& s1, float& sm) {
    const float fx0 = floorf(px), fy0 = floorf(py);
    const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    const float wnw = (fx1 - px) * (fy1 - py), wne = (px - fx0) * (fy1 - py);
    const float wsw = (fx1 - px) * (py - fy0), wse = (px - fx0) * (py - fy0);
    // clamped before the int conversion: a position far out of frame (or NaN: fmaxf returns the other operand) must not overflow it;
    // every clamped tap is outside
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f), y0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    float a0 = 0.f, a1 = 0.f, am = 0.f;
    auto tap = [&](int yy, int xx, float wt) {       // loads from a clamped address without a branch; only in-frame taps add
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const int q = in ? yy * w + xx : 0;
        const float v0 = c0[q], v1 = c1[q];
        a0 = in ? a0 + v0 * wt : a0;
        a1 = in ? a1 + v1 * wt : a1;
        if (m) {
            const float vm = m[q];
            am = in ? am + vm * wt : am;
        }
    };
    tap(y0, x0, wnw);
    tap(y0, x0 + 1, wne);
    tap(y0 + 1, x0, wsw);
    tap(y0 + 1, x0 + 1, wse);
    s0 = a0;
    s1 = a1;
    sm = am;
}

// 0 <= x <= w - 1 and 0 <= y <= h - 1; false for a NaN
__device__ __forceinline__ bool chain_inside(float x, float y, int h, int w) {
    return x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1);
}

// one thread per track: tracks[t][i] = position after pair t, visible[t][i] = still alive after pair t.  A lost track keeps the
// position of the step that lost it and samples nothing more.
__global__ __launch_bounds__(256) void flow_chain_kernel(const float* __restrict__ flow, const float* __restrict__ occ,
                                                         const float* __restrict__ pos_in, const unsigned char* __restrict__ alive_in,
                                                         f32x2* __restrict__ tracks, unsigned char* __restrict__ visible, int pairs,
                                                         int h, int w, int n, int gw, int stride) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long L = (long)h * w;
    float x, y;
    if (pos_in) {
        x = pos_in[2 * (long)i];
        y = pos_in[2 * (long)i + 1];
    } else {
        const int gy = i / gw;
        x = (float)((i - gy * gw) * stride);
        y = (float)(gy * stride);
    }
    bool alive = (alive_in ? alive_in[i] != 0 : true) && chain_inside(x, y, h, w);
    for (int t = 0; t < pairs; ++t) {
        if (alive) {
            const float* f = flow + (long)t * 2 * L;
            float u, v, o;
            chain_sample(f, f + L, occ ? occ + (long)t * L : nullptr, h, w, x, y, u, v, o);      // the mask at the OLD position
            x += u;
            y += v;
            alive = chain_inside(x, y, h, w) && !(o >= 0.5f);
        }
        f32x2 p;
        p[0] = x;
        p[1] = y;
        tracks[(long)t * n + i] = p;
        visible[(long)t * n + i] = alive ? 1 : 0;
    }
}

extern "C" int um_flow_chain(const float* flow, const float* occ, const float* pos_in, const unsigned char* alive_in, float* tracks,
                             unsigned char* visible, int pairs, int h, int w, int n, int grid_stride, void* stream) {
    const long lim = 1L << 30;
    if (!flow || !tracks || !visible || pairs <= 0 || n <= 0 || h < 2 || w < 2 || (long)h * w > lim || n > lim ||
        (long)pairs * n > lim || (long)pairs * h * w > lim || (uintptr_t)tracks % 8 != 0) {
        um_set_error("um_flow_chain: bad argument (pairs=%d h=%d w=%d n=%d)", pairs, h, w, n);
        return UM_ERR_BAD_ARG;
    }
    int gw = 1;
    if (!pos_in) {                                    // the start grid: every grid_stride-th pixel of every grid_stride-th row
        if (grid_stride < 1 || grid_stride > lim) {
            um_set_error("um_flow_chain: grid_stride %d (1 ... 2^30 when pos_in is null)", grid_stride);
            return UM_ERR_BAD_ARG;
        }
        gw = (w + grid_stride - 1) / grid_stride;
        const int gh = (h + grid_stride - 1) / grid_stride;
        if ((long)gw * gh != n) {
            um_set_error("um_flow_chain: n=%d, the stride-%d grid of %d x %d has %d x %d points", n, grid_stride, h, w, gh, gw);
            return UM_ERR_BAD_ARG;
        }
    }
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    hipLaunchKernelGGL(flow_chain_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flow, occ, pos_in,
                       alive_in, reinterpret_cast<f32x2*>(tracks), visible, pairs, h, w, n, gw, grid_stride);
    return (int)hipGetLastError();
}
