// Cross-view consistency masks and point clouds from predicted disparity / depth.                gfx950 / wave64
//
// Memory-bound, one thread per pixel, a workgroup never straddles two images (so the 30-float camera record of a pixel is uniform
// over its workgroup and is read through the scalar cache); nothing survives a call:
//
//   um_disp_consistency   left / right check of a rectified pair in ONE launch: forward_backward_consistency_check
//                         (unimatch/geometry.py:75-96) on the horizontal flows fwd = (-dL, 0), bwd = (+dR, 0), without the zero
//                         channel and without the two vertical taps: the other view's disparity is sampled linearly along the row.
//   um_depth_consistency  per pixel of a reference view: back_project, camera_transform and reproject (geometry.py:99-154) into the
//                         source view, bilinear sample of the source depth, the same three steps back with the inverse pose, and the
//                         two round-trip errors (pixels, relative depth).  One launch for any number of directed view pairs.
//   um_points_pack        stable compaction of the selected pixels of a batch of depth maps into a dense world-space point list
//                         (+ colours) in ascending (b, y, x) order.  Three deterministic launches -- per-workgroup counts (wave
//                         ballot + popcount), one workgroup's exclusive scan of the counts, scatter at offset + rank -- and no
//                         atomics: row n is the n-th selected pixel, every call.
//
// Compiled with -ffp-contract=off and correctly rounded division / square root (build.py): every product, sum and quotient is
// rounded on its own, in the order the host restatement of unimatch_amd/geometry.py evaluates them.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

#define UM_GEO_WG 256                          // threads = pixels per workgroup (four waves)
#define UM_GEO_SCAN_WG 1024                    // threads of the single scan workgroup (sixteen waves)

static inline bool geo_sizes_ok(int batch, int h, int w) {
    return batch > 0 && h > 0 && w > 0 && (long)batch * h * w < (1L << 31);
}

static inline long geo_chunks(int h, int w) { return ((long)h * w + UM_GEO_WG - 1) / UM_GEO_WG; }

// ---- disparity: left / right check ----------------------------------------------------------------------------------------------

// grid_sample(align_corners=True, zeros) of one row at x + dx, with the coordinate round trip of occ_sample (video.hip): the
// vertical coordinate of a horizontal flow is the row itself, so only the two taps of that row remain.
__device__ __forceinline__ float row_sample(const float* __restrict__ row, int w, int x, float dx) {
    const float px = (float)x + dx;
    const float gx = 2.0f * px / (float)(w - 1) - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(w - 1);
    const float fx0 = floorf(ix), fx1 = fx0 + 1.0f;
    const float w0 = fx1 - ix, w1 = ix - fx0;
    // clamped before the int conversion: a disparity far out of frame (or NaN) must not overflow it; every clamped tap is outside
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f);
    const bool in0 = x0 >= 0 && x0 < w, in1 = x0 + 1 >= 0 && x0 + 1 < w;
    const float v0 = row[in0 ? x0 : 0], v1 = row[in1 ? x0 + 1 : 0];      // loads from a clamped address; only in-frame taps add
    float a = 0.f;
    a = in0 ? a + v0 * w0 : a;
    a = in1 ? a + v1 * w1 : a;
    return a;
}

__global__ __launch_bounds__(UM_GEO_WG) void disp_consistency_kernel(const float* __restrict__ dl, const float* __restrict__ dr,
                                                                     float* __restrict__ occ_l, float* __restrict__ occ_r, int h, int w,
                                                                     int chunks, float alpha, float beta) {
    const int L = h * w;
    const int b = blockIdx.x / chunks;
    const int p = (blockIdx.x - b * chunks) * UM_GEO_WG + threadIdx.x;
    if (p >= L) return;
    const int y = p / w, x = p - y * w;
    const long i = (long)b * L + p;
    const float* rl = dl + (long)b * L + (long)y * w;
    const float* rr = dr + (long)b * L + (long)y * w;
    const float fu = -rl[x], bu = rr[x];                      // the horizontal flows of the two views
    const float wbu = row_sample(rr, w, x, fu);               // right disparity seen from the left pixel's match
    const float wfu = row_sample(rl, w, x, bu);               // (minus) left disparity seen from the right pixel's match
    const float mag = __fsqrt_rn(fu * fu) + __fsqrt_rn(bu * bu);
    const float thr = alpha * mag + beta;
    const float du = fu + wbu, eu = bu - wfu;
    occ_l[i] = __fsqrt_rn(du * du) > thr ? 1.f : 0.f;
    occ_r[i] = __fsqrt_rn(eu * eu) > thr ? 1.f : 0.f;
}

extern "C" int um_disp_consistency(const float* disp_left, const float* disp_right, float* occ_left, float* occ_right, int batch, int h,
                                   int w, float alpha, float beta, void* stream) {
    if (!disp_left || !disp_right || !occ_left || !occ_right || !geo_sizes_ok(batch, h, w) || w < 2) {
        um_set_error("um_disp_consistency: bad argument (batch=%d h=%d w=%d)", batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    const long chunks = geo_chunks(h, w);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    hipLaunchKernelGGL(disp_consistency_kernel, dim3((unsigned)(chunks * batch)), dim3(UM_GEO_WG), 0, (hipStream_t)stream, disp_left,
                       disp_right, occ_left, occ_right, h, w, (int)chunks, alpha, beta);
    return (int)hipGetLastError();
}

// ---- depth: round trip through the other view -----------------------------------------------------------------------------------

// X = R (depth Kinv [u v 1]^T) + t of a cam record (Kinv | R | t | K); the operation order of rigid_flow_kernel (upsample.hip)
__device__ __forceinline__ void cam_lift(const float* __restrict__ cm, float u, float v, float depth, float& X, float& Y, float& Z) {
    const float r0 = (cm[0] * u + cm[1] * v + cm[2]) * depth, r1 = (cm[3] * u + cm[4] * v + cm[5]) * depth,
                r2 = (cm[6] * u + cm[7] * v + cm[8]) * depth;
    X = cm[9] * r0 + cm[10] * r1 + cm[11] * r2 + cm[18];
    Y = cm[12] * r0 + cm[13] * r1 + cm[14] * r2 + cm[19];
    Z = cm[15] * r0 + cm[16] * r1 + cm[17] * r2 + cm[20];
}

// (u, v) = (K X)_xy / max((K X)_z, 1e-3): reproject (geometry.py:132-154)
__device__ __forceinline__ void cam_project(const float* __restrict__ cm, float X, float Y, float Z, float& u, float& v) {
    const float pu = cm[21] * X + cm[22] * Y + cm[23] * Z, pv = cm[24] * X + cm[25] * Y + cm[26] * Z;
    const float zz = fmaxf(cm[27] * X + cm[28] * Y + cm[29] * Z, 1e-3f);
    u = pu / zz;
    v = pv / zz;
}

__device__ __forceinline__ bool depth_ok(float d) { return d > 0.f && d <= 3.402823466e+38f; }      // finite and positive (false for NaN)

__global__ __launch_bounds__(UM_GEO_WG) void depth_consistency_kernel(const float* __restrict__ depth_ref, const float* __restrict__ depth_src,
                                                                      const float* __restrict__ cam_fwd, const float* __restrict__ cam_inv,
                                                                      float* __restrict__ occ, float* __restrict__ err_px,
                                                                      float* __restrict__ err_rel, int h, int w, int chunks, float px_thr,
                                                                      float rel_thr) {
    const int L = h * w;
    const int b = blockIdx.x / chunks;
    const int p = (blockIdx.x - b * chunks) * UM_GEO_WG + threadIdx.x;
    if (p >= L) return;
    const int y = p / w, x = p - y * w;
    const long i = (long)b * L + p;
    const float* cf = cam_fwd + (long)b * 30;
    const float* ci = cam_inv + (long)b * 30;
    const float* src = depth_src + (long)b * L;
    const float gx = (float)x, gy = (float)y;
    const float d = depth_ref[i];
    const float inf = __builtin_inff();
    float epx = inf, erel = inf;
    float X, Y, Z, u, v;
    cam_lift(cf, gx, gy, d, X, Y, Z);
    cam_project(cf, X, Y, Z, u, v);
    // in view (false for NaN); the conversions below are then in range
    const bool in = depth_ok(d) && u >= 0.f && u <= (float)(w - 1) && v >= 0.f && v <= (float)(h - 1);
    const float fx0 = in ? floorf(u) : 0.f, fy0 = in ? floorf(v) : 0.f;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float ax = in ? u - fx0 : 0.f, ay = in ? v - fy0 : 0.f;
    const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
    // four taps from clamped (in-frame) addresses; a tap of weight zero neither adds nor invalidates
    const float t00 = src[y0 * w + x0], t01 = src[y0 * w + x1], t10 = src[y1 * w + x0], t11 = src[y1 * w + x1];
    bool ok = in;
    float s = 0.f;
    auto tap = [&](float t, float wt) {
        const bool used = wt != 0.f;
        ok = ok && (!used || depth_ok(t));
        s = used ? s + wt * t : s;
    };
    tap(t00, w00);
    tap(t01, w01);
    tap(t10, w10);
    tap(t11, w11);
    if (ok) {
        float bu, bv;
        cam_lift(ci, u, v, s, X, Y, Z);                       // the sampled source point, in the reference camera
        cam_project(ci, X, Y, Z, bu, bv);
        const float ex = bu - gx, ey = bv - gy;
        epx = __fsqrt_rn(ex * ex + ey * ey);
        erel = fabsf(Z - d) / d;
    }
    occ[i] = (epx < px_thr && erel < rel_thr) ? 0.f : 1.f;
    if (err_px) err_px[i] = epx;
    if (err_rel) err_rel[i] = erel;
}

extern "C" int um_depth_consistency(const float* depth_ref, const float* depth_src, const float* cam_fwd, const float* cam_inv, float* occ,
                                    float* err_px, float* err_rel, int batch, int h, int w, float px_thr, float rel_thr, void* stream) {
    if (!depth_ref || !depth_src || !cam_fwd || !cam_inv || !occ || !geo_sizes_ok(batch, h, w)) {
        um_set_error("um_depth_consistency: bad argument (batch=%d h=%d w=%d)", batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    const long chunks = geo_chunks(h, w);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    hipLaunchKernelGGL(depth_consistency_kernel, dim3((unsigned)(chunks * batch)), dim3(UM_GEO_WG), 0, (hipStream_t)stream, depth_ref,
                       depth_src, cam_fwd, cam_inv, occ, err_px, err_rel, h, w, (int)chunks, px_thr, rel_thr);
    return (int)hipGetLastError();
}

// ---- points: stable compaction --------------------------------------------------------------------------------------------------

// is pixel p of image b selected, and its depth
__device__ __forceinline__ bool point_selected(const float* __restrict__ depth, const float* __restrict__ keep, long i, int p, int L,
                                               int w, int stride, float min_depth, float max_depth, float& d) {
    if (p >= L) return false;
    const int y = p / w, x = p - y * w;
    if (x % stride != 0 || y % stride != 0) return false;
    if (keep && keep[i] == 0.f) return false;
    d = depth[i];
    return d > min_depth && d < max_depth && d <= 3.402823466e+38f && d >= -3.402823466e+38f;        // false for NaN and +-inf
}

// phase 1: counts[workgroup] = number of selected pixels of the workgroup's 256
__global__ __launch_bounds__(UM_GEO_WG) void points_count_kernel(const float* __restrict__ depth, const float* __restrict__ keep,
                                                                 int* __restrict__ counts, int h, int w, int chunks, int stride,
                                                                 float min_depth, float max_depth) {
    __shared__ int wave_n[UM_GEO_WG / 64];
    const int L = h * w;
    const int b = blockIdx.x / chunks;
    const int p = (blockIdx.x - b * chunks) * UM_GEO_WG + threadIdx.x;
    float d;
    const bool sel = point_selected(depth, keep, (long)b * L + p, p, L, w, stride, min_depth, max_depth, d);
    const unsigned long long mask = __ballot(sel);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// phase 2: offsets[i] = counts[0] + ... + counts[i - 1], total[0] = the sum of all; one workgroup, each thread a contiguous run
__global__ __launch_bounds__(UM_GEO_SCAN_WG) void points_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                                     int* __restrict__ total, int n) {
    __shared__ int wave_sum[UM_GEO_SCAN_WG / 64];
    const int per = (n + UM_GEO_SCAN_WG - 1) / UM_GEO_SCAN_WG;
    const long lo = (long)threadIdx.x * per;
    const long hi = lo + per < (long)n ? lo + per : (long)n;
    int s = 0;
    for (long i = lo; i < hi; ++i) s += counts[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        incl = lane >= o ? incl + up : incl;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wave; ++k) before += wave_sum[k];
    int run = before + incl - s;
    for (long i = lo; i < hi; ++i) {
        const int c = counts[i];
        offsets[i] = run;
        run += c;
    }
    if (threadIdx.x == UM_GEO_SCAN_WG - 1) total[0] = before + incl;
}

// phase 3: row (offset of the workgroup + rank inside it) of every selected pixel
__global__ __launch_bounds__(UM_GEO_WG) void points_scatter_kernel(const float* __restrict__ depth, const float* __restrict__ cam,
                                                                   const float* __restrict__ keep, const unsigned char* __restrict__ colors,
                                                                   const int* __restrict__ offsets, float* __restrict__ xyz,
                                                                   unsigned char* __restrict__ rgb, int h, int w, int chunks, int stride,
                                                                   float min_depth, float max_depth) {
    __shared__ int wave_n[UM_GEO_WG / 64];
    const int L = h * w;
    const int b = blockIdx.x / chunks;
    const int p = (blockIdx.x - b * chunks) * UM_GEO_WG + threadIdx.x;
    const long i = (long)b * L + p;
    float d = 0.f;
    const bool sel = point_selected(depth, keep, i, p, L, w, stride, min_depth, max_depth, d);
    const unsigned long long mask = __ballot(sel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    if (!sel) return;
    int row = offsets[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) row += wave_n[k];
    const int y = p / w, x = p - y * w;
    float X, Y, Z;
    cam_lift(cam + (long)b * 30, (float)x, (float)y, d, X, Y, Z);
    float* o = xyz + (long)row * 3;
    o[0] = X;
    o[1] = Y;
    o[2] = Z;
    if (rgb) {
        const unsigned char* c = colors + i * 3;
        unsigned char* q = rgb + (long)row * 3;
        q[0] = c[0];
        q[1] = c[1];
        q[2] = c[2];
    }
}

static inline bool points_args_ok(int batch, int h, int w, int stride) { return geo_sizes_ok(batch, h, w) && stride > 0; }

extern "C" size_t um_points_workspace_bytes(int batch, int h, int w, int stride) {
    if (!points_args_ok(batch, h, w, stride)) return 0;
    return (size_t)(geo_chunks(h, w) * batch) * 2 * sizeof(int);          // counts | offsets
}

extern "C" int um_points_pack(const float* depth, const float* cam_world, const float* keep, const unsigned char* colors, float* xyz,
                              unsigned char* rgb, int* count, int batch, int h, int w, int stride, float min_depth, float max_depth,
                              void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!depth || !cam_world || !xyz || !count || (colors == nullptr) != (rgb == nullptr) || !points_args_ok(batch, h, w, stride)) {
        um_set_error("um_points_pack: bad argument (batch=%d h=%d w=%d stride=%d; colors and rgb go together)", batch, h, w, stride);
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_points_workspace_bytes(batch, h, w, stride);
    if (!workspace || ws_bytes < need || (uintptr_t)workspace % sizeof(int) != 0) {
        um_set_error("um_points_pack: workspace of %zu bytes, %zu needed (4-byte aligned)", ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const long chunks = geo_chunks(h, w);
    const int n = (int)(chunks * batch);
    int* counts = (int*)workspace;
    int* offsets = counts + n;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(points_count_kernel, dim3((unsigned)n), dim3(UM_GEO_WG), 0, stream, depth, keep, counts, h, w, (int)chunks, stride,
                       min_depth, max_depth);
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(UM_GEO_SCAN_WG), 0, stream, (const int*)counts, offsets, count, n);
    hipLaunchKernelGGL(points_scatter_kernel, dim3((unsigned)n), dim3(UM_GEO_WG), 0, stream, depth, cam_world, keep, colors,
                       (const int*)offsets, xyz, rgb, h, w, (int)chunks, stride, min_depth, max_depth);
    return (int)hipGetLastError();
}
