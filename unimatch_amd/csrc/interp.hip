// Frame synthesis from flow: image warp, forward flow splat, in-between frames.                               gfx950 / wave64
//
// A classical synthesis without any learned part: the flows of a pair are moved to the time t by forward splatting (flow reversal),
// both frames are warped backwards by the splatted motion and blended with occlusion-aware weights.  Three entry points, all
// memory-bound, one thread per pixel, nothing kept between calls:
//
//   um_image_warp        out(p) = bilinear(image, p + flow(p)): the reference's flow_warp (unimatch/geometry.py:41-72) applied to an
//                        IMAGE (any channel count in fp32 NCHW, or uint8 NHWC frames as a decoder delivers them), zeros or border
//                        padding, with the reference's return_mask.  The taps are computed once per pixel and reused per channel.
//   um_flow_splat        every source pixel p of a flow lands at p + t flow(p) for each of K times and adds its flow to the four
//                        pixels around the landing point, weighted bilinearly.  This is the one kernel of the library that sums
//                        across threads into arbitrary destinations, and it does so in INTEGERS: the weight is quantised to 2^-16,
//                        the flow to 2^-8 px, and three int64 planes per (direction, batch, time) receive sum w, sum w u, sum w v by
//                        64-bit integer atomic adds.  Integer adds commute, so the sums do not depend on the order the adds arrive in:
//                        the result is bitwise reproducible and bitwise equal to the host restatement (interp.py), which float
//                        atomics cannot give.  The entry point clears the accumulators on the caller's stream before the launch.
//   um_frame_synthesize  per output pixel and time: normalise both directions' accumulators in float64, combine them into one motion
//                        estimate, sample both frames (border clamping) and both occlusion masks (zeros outside), blend, round.
//
// Budget of the splat (one (direction, t) at 1080 x 1920): 2.07 M pixels x 4 taps x 3 planes x 8 B = 199 MB of added bytes.  At the
// chip-wide rate measured for float atomics (about 1.3 TB/s of added bytes) that is 0.15 ms.  Measured for these 64-bit integer adds
// (tools/bench_interpolate.py, profiles/interpolate.txt): 1.07 - 1.13 TB/s over the whole call, its clear included -- 0.18 ms per
// (direction, t) at 1080 x 1920, so the launch runs at the atomic rate.  Lanes of a wave hold neighbouring pixels of a row, so under a
// smooth flow one wave-instruction adds into a few contiguous runs of a row of one plane: the favourable access shape.  The planes stay
// planar: the cost is added bytes, which an interleaved [H W][4] layout would not reduce.
//
// Largest sum: |u| <= 32768 px gives |uq| <= 2^23, wq <= 2^16, and a destination receives at most one tap of each source pixel, so
// |S| <= H W 2^39.  The entry points cap H W at 2^21: |S| <= 2^60 < 2^63.
//
// Compiled with -ffp-contract=off and correctly rounded division (build.py): the host restatement rounds every product, sum and
// quotient on its own, and the two are compared bit for bit.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

#define UM_SPLAT_MAX_PX (1L << 21)
#define UM_SPLAT_MAX_FLOW 32768.0f
#define UM_SPLAT_WEIGHT_ONE 65536.0f
#define UM_SPLAT_FLOW_ONE 256.0f

// the times of a call, by value: row 0 for the forward direction, row 1 for the backward one
struct InterpTimes {
    float t[2][UM_INTERP_MAX_TIMES];
};

// ---- gather ---------------------------------------------------------------------------------------------------------------------

// the four taps around the position (ix, iy): weights and tap order of occ_sample (csrc/video.hip)
struct Taps {
    float wnw, wne, wsw, wse;
    int x0, y0;
};

__device__ __forceinline__ Taps make_taps(float ix, float iy, int h, int w) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    Taps t;
    t.wnw = (fx1 - ix) * (fy1 - iy);
    t.wne = (ix - fx0) * (fy1 - iy);
    t.wsw = (fx1 - ix) * (iy - fy0);
    t.wse = (ix - fx0) * (iy - fy0);
    // clamped before the int conversion: a position far out of frame (or NaN: fmaxf returns the other operand) must not overflow it;
    // every clamped tap is outside
    t.x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f);
    t.y0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    return t;
}

// into the frame: a NaN goes to 0
__device__ __forceinline__ float clamp_pos(float p, int n) { return fminf(fmaxf(p, 0.f), (float)(n - 1)); }

// 0 <= x <= w - 1 and 0 <= y <= h - 1; false for a NaN
__device__ __forceinline__ bool pos_inside(float x, float y, int h, int w) {
    return x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1);
}

// one channel of image b at pixel q: [B][C][L] fp32 or [B][L][C] uint8
template <bool U8>
__device__ __forceinline__ float image_at(const void* __restrict__ image, long b, int channels, long L, int c, int q) {
    if (U8) return (float)reinterpret_cast<const unsigned char*>(image)[(b * L + q) * channels + c];
    return reinterpret_cast<const float*>(image)[(b * channels + c) * L + q];
}

// sum of the in-frame taps of channel c, NW, NE, SW, SE; loads from a clamped address without a branch
template <bool U8>
__device__ __forceinline__ float gather(const void* __restrict__ image, long b, int channels, int h, int w, int c, const Taps& t) {
    const long L = (long)h * w;
    float a = 0.f;
    auto tap = [&](int yy, int xx, float wt) {
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const float v = image_at<U8>(image, b, channels, L, c, in ? yy * w + xx : 0);
        a = in ? a + v * wt : a;
    };
    tap(t.y0, t.x0, t.wnw);
    tap(t.y0, t.x0 + 1, t.wne);
    tap(t.y0 + 1, t.x0, t.wsw);
    tap(t.y0 + 1, t.x0 + 1, t.wse);
    return a;
}

__device__ __forceinline__ unsigned char to_byte(float v) { return (unsigned char)(int)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// ---- um_image_warp --------------------------------------------------------------------------------------------------------------

template <bool U8>
__global__ __launch_bounds__(256) void image_warp_kernel(const void* __restrict__ image, const float* __restrict__ flow,
                                                         void* __restrict__ out, unsigned char* __restrict__ mask, int channels, int h,
                                                         int w, int border) {
    const int L = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const long b = blockIdx.y;
    const int y = p / w, x = p - y * w;
    const float* f = flow + b * 2 * L;
    const float px = (float)x + f[p], py = (float)y + f[L + p];
    // the reference's coordinate round trip: normalise (geometry.py:52-53), un-normalise inside grid_sample
    const float gx = 2.0f * px / (float)(w - 1) - 1.0f, gy = 2.0f * py / (float)(h - 1) - 1.0f;
    float ix = ((gx + 1.0f) / 2.0f) * (float)(w - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(h - 1);
    if (mask) mask[b * L + p] = (gx >= -1.0f && gy >= -1.0f && gx <= 1.0f && gy <= 1.0f) ? 1 : 0;
    if (border) {
        ix = clamp_pos(ix, w);
        iy = clamp_pos(iy, h);
    }
    const Taps t = make_taps(ix, iy, h, w);
    for (int c = 0; c < channels; ++c) {
        const float a = gather<U8>(image, b, channels, h, w, c, t);
        if (U8)
            reinterpret_cast<unsigned char*>(out)[(b * L + p) * channels + c] = to_byte(a);
        else
            reinterpret_cast<float*>(out)[(b * channels + c) * L + p] = a;
    }
}

extern "C" int um_image_warp(const void* image, int layout, const float* flow, void* out, unsigned char* mask, int batch, int channels,
                             int h, int w, int border, void* stream) {
    const bool u8 = layout == UM_IMG_U8_NHWC;
    if (!image || !flow || !out || (layout != UM_IMG_F32_NCHW && layout != UM_IMG_U8_NHWC) || batch <= 0 || batch > 65535 ||
        channels < 1 || channels > 65535 || (u8 && channels != 3) || h < 2 || w < 2 || (long)h * w > (1L << 30) ||
        (long)batch * channels * h * w > (1L << 40)) {
        um_set_error("um_image_warp: bad argument (layout=%d batch=%d channels=%d h=%d w=%d)", layout, batch, channels, h, w);
        return UM_ERR_BAD_ARG;
    }
    const long L = (long)h * w;
    const dim3 grid((unsigned)((L + 255) / 256), (unsigned)batch);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    if (u8)
        hipLaunchKernelGGL(image_warp_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, image, flow, out, mask, channels, h, w,
                           border ? 1 : 0);
    else
        hipLaunchKernelGGL(image_warp_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, image, flow, out, mask, channels, h, w,
                           border ? 1 : 0);
    return (int)hipGetLastError();
}

// ---- um_flow_splat --------------------------------------------------------------------------------------------------------------

// accumulators: [dirs][batch][k][3][L] int64, planes S_w, S_u, S_v
__device__ __forceinline__ long acc_offset(int dir, int batch, long b, int k, int kk, long L) {
    return (((long)dir * batch + b) * k + kk) * 3 * L;
}

__device__ __forceinline__ void add64(unsigned long long* p, long long v) {
    __hip_atomic_fetch_add(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void flow_splat_kernel(const float* __restrict__ flow_fwd, const float* __restrict__ flow_bwd,
                                                         const float* __restrict__ weight_fwd, const float* __restrict__ weight_bwd,
                                                         unsigned long long* __restrict__ acc, InterpTimes times, int batch, int k,
                                                         int h, int w) {
    const int L = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const long b = blockIdx.y;
    const int dir = blockIdx.z;
    const float* f = (dir ? flow_bwd : flow_fwd) + b * 2 * L;
    const float* wgt = dir ? weight_bwd : weight_fwd;
    const float u = f[p], v = f[L + p];
    if (!(fabsf(u) <= UM_SPLAT_MAX_FLOW) || !(fabsf(v) <= UM_SPLAT_MAX_FLOW)) return;        // NaN, inf, out of range: nothing
    float g = 1.0f;
    if (wgt) {
        g = wgt[b * L + p];
        if (!(g > 0.f) || g == __builtin_inff()) return;                                     // NaN, inf, <= 0: nothing
        g = fminf(g, 1.0f);
    }
    const long long uq = llrintf(u * UM_SPLAT_FLOW_ONE), vq = llrintf(v * UM_SPLAT_FLOW_ONE);
    const int y = p / w, x = p - y * w;
    for (int kk = 0; kk < k; ++kk) {
        const float t = times.t[dir][kk];
        const float X = (float)x + t * u, Y = (float)y + t * v;                              // |X| < 2^21 + 2^15: the int conversion is safe
        const float fx0 = floorf(X), fy0 = floorf(Y);
        const float ax = X - fx0, ay = Y - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        unsigned long long* base = acc + acc_offset(dir, batch, b, k, kk, L);
        auto tap = [&](int yy, int xx, float wt) {
            const long long wq = llrintf((wt * g) * UM_SPLAT_WEIGHT_ONE);
            if (yy >= 0 && yy < h && xx >= 0 && xx < w && wq > 0) {
                const int q = yy * w + xx;
                add64(base + q, wq);
                add64(base + L + q, wq * uq);
                add64(base + 2L * L + q, wq * vq);
            }
        };
        tap(y0, x0, (1.0f - ax) * (1.0f - ay));
        tap(y0, x0 + 1, ax * (1.0f - ay));
        tap(y0 + 1, x0, (1.0f - ax) * ay);
        tap(y0 + 1, x0 + 1, ax * ay);
    }
}

// the splatted flow of one pixel: false (and zero flow) where the summed weight is below thr (>= 1)
__device__ __forceinline__ bool splat_value(const long long* __restrict__ base, long L, int p, long long thr, float& u, float& v) {
    const long long sw = base[p];
    const bool ok = sw >= thr;
    const double den = ok ? (double)sw : 1.0;
    const float uu = (float)((double)base[L + p] / den / 256.0), vv = (float)((double)base[2 * L + p] / den / 256.0);
    u = ok ? uu : 0.f;
    v = ok ? vv : 0.f;
    return ok;
}

// optional second launch: avg [dirs][batch][k][2][L] fp32 and hole [dirs][batch][k][L] bytes from the accumulators
__global__ __launch_bounds__(256) void splat_normalize_kernel(const long long* __restrict__ acc, float* __restrict__ avg,
                                                              unsigned char* __restrict__ hole, long long thr, int L) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const long plane = blockIdx.y;                       // (dir, b, kk) flattened: the accumulators are laid out in that order
    float u, v;
    const bool ok = splat_value(acc + plane * 3 * L, L, p, thr, u, v);
    if (avg) {
        avg[plane * 2 * L + p] = u;
        avg[plane * 2 * L + L + p] = v;
    }
    if (hole) hole[plane * L + p] = ok ? 0 : 1;
}

static inline bool splat_dims_ok(int batch, int dirs, int k, int h, int w) {
    return batch > 0 && batch <= 65535 && (dirs == 1 || dirs == 2) && k >= 1 && k <= UM_INTERP_MAX_TIMES && h >= 2 && w >= 2 &&
           (long)h * w <= UM_SPLAT_MAX_PX && (long)batch * dirs * k <= 65535;
}

static inline bool times_ok(const float* times, int n) {
    for (int i = 0; i < n; ++i)
        if (!(times[i] > 0.f && times[i] < 1.f)) return false;
    return true;
}

// rint(min_weight 65536) in float32, at least 1: a pixel that received nothing is always a hole
static inline long long hole_threshold(float min_weight) {
    const long long thr = llrintf(min_weight * UM_SPLAT_WEIGHT_ONE);
    return thr < 1 ? 1 : thr;
}

extern "C" size_t um_flow_splat_workspace_bytes(int batch, int dirs, int k, int h, int w) {
    if (!splat_dims_ok(batch, dirs, k, h, w)) return 0;
    return (size_t)batch * dirs * k * 3 * (size_t)h * w * sizeof(long long);
}

extern "C" int um_flow_splat(const float* flow_fwd, const float* flow_bwd, const float* weight_fwd, const float* weight_bwd,
                             const float* times, int batch, int k, int h, int w, float min_weight, float* avg_out,
                             unsigned char* hole_out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int dirs = flow_bwd ? 2 : 1;
    if (!flow_fwd || !times || !workspace || (weight_bwd && !flow_bwd) || !splat_dims_ok(batch, dirs, k, h, w) ||
        (uintptr_t)workspace % 8 != 0 || !(min_weight >= 0.f && min_weight <= 1.f)) {
        um_set_error("um_flow_splat: bad argument (batch=%d k=%d h=%d w=%d min_weight=%g; k <= %d, h, w >= 2, h * w <= 2^21)", batch, k,
                     h, w, (double)min_weight, UM_INTERP_MAX_TIMES);
        return UM_ERR_BAD_ARG;
    }
    if (!times_ok(times, dirs * k)) {
        um_set_error("um_flow_splat: every time must lie strictly between 0 and 1");
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_flow_splat_workspace_bytes(batch, dirs, k, h, w);
    if (ws_bytes < need) {
        um_set_error("um_flow_splat: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return UM_ERR_BAD_ARG;
    }
    InterpTimes tt = {};
    for (int d = 0; d < dirs; ++d)
        for (int i = 0; i < k; ++i) tt.t[d][i] = times[d * k + i];
    const int L = h * w;
    const unsigned blocks = (unsigned)((L + 255) / 256);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    // cleared by every call, on the caller's stream: no launch ever reads what an earlier call left behind
    hipError_t err = hipMemsetAsync(workspace, 0, need, stream);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(flow_splat_kernel, dim3(blocks, (unsigned)batch, (unsigned)dirs), dim3(256), 0, stream, flow_fwd, flow_bwd,
                       weight_fwd, weight_bwd, (unsigned long long*)workspace, tt, batch, k, h, w);
    if (avg_out || hole_out)
        hipLaunchKernelGGL(splat_normalize_kernel, dim3(blocks, (unsigned)(batch * dirs * k)), dim3(256), 0, stream,
                           (const long long*)workspace, avg_out, hole_out, hole_threshold(min_weight), L);
    return (int)hipGetLastError();
}

// ---- um_frame_synthesize --------------------------------------------------------------------------------------------------------

// bilinear sample of one mask plane at (px, py), zeros outside
__device__ __forceinline__ float mask_sample(const float* __restrict__ m, long b, int h, int w, float px, float py) {
    if (!m) return 0.f;
    const Taps t = make_taps(px, py, h, w);
    return gather<false>(m, b, 1, h, w, 0, t);
}

template <bool U8>
__global__ __launch_bounds__(256) void frame_synth_kernel(const void* __restrict__ img0, const void* __restrict__ img1,
                                                          const float* __restrict__ occ_fwd, const float* __restrict__ occ_bwd,
                                                          const long long* __restrict__ acc, unsigned char* __restrict__ out,
                                                          unsigned char* __restrict__ holes, InterpTimes times, long long thr,
                                                          int batch, int k, int h, int w) {
    const int L = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const long b = blockIdx.y;
    const int kk = blockIdx.z;
    const int y = p / w, x = p - y * w;
    const float t = times.t[0][kk], t1 = times.t[1][kk];                 // t and 1 - t (the time of the backward splat)
    float au, av, bu, bv;
    const bool va = splat_value(acc + acc_offset(0, batch, b, k, kk, L), L, p, thr, au, av);
    const bool vb = splat_value(acc + acc_offset(1, batch, b, k, kk, L), L, p, thr, bu, bv);
    float mu = 0.f, mv = 0.f;
    if (va && vb) {
        mu = 0.5f * (au + (-bu));
        mv = 0.5f * (av + (-bv));
    } else if (va) {
        mu = au;
        mv = av;
    } else if (vb) {
        mu = -bu;
        mv = -bv;
    }
    const float x0 = (float)x - t * mu, y0 = (float)y - t * mv;          // where q comes from in frame 0
    const float x1 = (float)x + t1 * mu, y1 = (float)y + t1 * mv;        // where q goes to in frame 1
    const bool v0 = pos_inside(x0, y0, h, w), v1 = pos_inside(x1, y1, h, w);
    const Taps ta = make_taps(clamp_pos(x0, w), clamp_pos(y0, h), h, w), tb = make_taps(clamp_pos(x1, w), clamp_pos(y1, h), h, w);
    const float o0 = mask_sample(occ_fwd, b, h, w, x0, y0), o1 = mask_sample(occ_bwd, b, h, w, x1, y1);
    float w0 = v0 ? t1 * (1.0f - o1) : 0.f, w1 = v1 ? t * (1.0f - o0) : 0.f;
    float ws = w0 + w1;
    if (!(ws >= 1e-6f)) {
        w0 = t1;
        w1 = t;
        ws = w0 + w1;
    }
    unsigned char* o = out + ((b * k + kk) * L + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float c0 = gather<U8>(img0, b, 3, h, w, c, ta), c1 = gather<U8>(img1, b, 3, h, w, c, tb);
        o[c] = to_byte((w0 * c0 + w1 * c1) / ws);
    }
    if (holes) holes[(b * k + kk) * L + p] = (va || vb) ? 0 : 1;
}

extern "C" int um_frame_synthesize(const void* img0, const void* img1, int layout, const float* occ_fwd, const float* occ_bwd,
                                   const float* times, const void* accum, size_t accum_bytes, unsigned char* out, unsigned char* holes,
                                   int batch, int k, int h, int w, float min_weight, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!img0 || !img1 || !times || !accum || !out || (layout != UM_IMG_F32_NCHW && layout != UM_IMG_U8_NHWC) ||
        !splat_dims_ok(batch, 2, k, h, w) || (uintptr_t)accum % 8 != 0 || !(min_weight >= 0.f && min_weight <= 1.f)) {
        um_set_error("um_frame_synthesize: bad argument (layout=%d batch=%d k=%d h=%d w=%d min_weight=%g; k <= %d, h, w >= 2, "
                     "h * w <= 2^21)", layout, batch, k, h, w, (double)min_weight, UM_INTERP_MAX_TIMES);
        return UM_ERR_BAD_ARG;
    }
    if (!times_ok(times, 2 * k)) {
        um_set_error("um_frame_synthesize: every time must lie strictly between 0 and 1");
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_flow_splat_workspace_bytes(batch, 2, k, h, w);
    if (accum_bytes < need) {
        um_set_error("um_frame_synthesize: accumulators of %zu bytes, %zu needed", accum_bytes, need);
        return UM_ERR_BAD_ARG;
    }
    InterpTimes tt = {};
    for (int d = 0; d < 2; ++d)
        for (int i = 0; i < k; ++i) tt.t[d][i] = times[d * k + i];
    const int L = h * w;
    const dim3 grid((unsigned)((L + 255) / 256), (unsigned)batch, (unsigned)k);
    const long long thr = hole_threshold(min_weight);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    if (layout == UM_IMG_U8_NHWC)
        hipLaunchKernelGGL(frame_synth_kernel<true>, grid, dim3(256), 0, stream, img0, img1, occ_fwd, occ_bwd, (const long long*)accum,
                           out, holes, tt, thr, batch, k, h, w);
    else
        hipLaunchKernelGGL(frame_synth_kernel<false>, grid, dim3(256), 0, stream, img0, img1, occ_fwd, occ_bwd, (const long long*)accum,
                           out, holes, tt, thr, batch, k, h, w);
    return (int)hipGetLastError();
}
