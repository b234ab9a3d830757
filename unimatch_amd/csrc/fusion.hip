// Volumetric (truncated signed distance) fusion of posed depth maps, and the surface points of the fused volume.   gfx950 / wave64
//
// One thread per voxel, the volume caller-owned (tsdf, weight [nz,ny,nx] fp32, colour planes [3,nz,ny,nx] fp32, x fastest); nothing
// survives a call and there are no atomics.  The integration crosses the volume once per call and is bound by its arithmetic (the IEEE
// quotients of the projection and of the running means: profiles/tsdf.txt), the extraction by memory:
//
//   um_tsdf_integrate   ONE launch applies all B views to every voxel in ascending b with the running (tsdf, weight, colour) held in
//                       registers: the volume is read once and written once per call whatever B is, and the result is the same as B
//                       one-view calls, bit for bit.  A wave covers 64 consecutive i of one (j, k) row -- full 256-byte segments of
//                       the volume -- the 30-float camera record of a view is uniform over the launch (scalar loads), and the depth
//                       reads are gathers with strong locality: neighbouring voxels project to neighbouring pixels.
//   um_tsdf_points      stable compaction of the zero crossings along the three axes into a dense point list (+ colours) in ascending
//                       (k, j, i, axis) order, built as um_points_pack (geometry.hip) is: per-workgroup counts (wave ballot +
//                       popcount), one workgroup's exclusive scan, scatter at offset + rank.
//
// Compiled with -ffp-contract=off and correctly rounded division (build.py): every product, sum and quotient is rounded on its own, in
// the order the host restatement of unimatch_amd/fusion.py evaluates them.
#include "common.h"
#include "timing.h"
#include "tsdf_grid.h"

extern void um_set_error(const char* fmt, ...);

#define UM_TSDF_WG 256                         // threads = voxels per workgroup (four waves)
#define UM_TSDF_SCAN_WG 1024                   // threads of the single scan workgroup (sixteen waves)
#define UM_TSDF_FLT_MAX 3.402823466e+38f

__device__ __forceinline__ bool tsdf_finite(float v) { return v <= UM_TSDF_FLT_MAX && v >= -UM_TSDF_FLT_MAX; }       // false for NaN

// ---- integrate ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(UM_TSDF_WG) void tsdf_integrate_kernel(const float* __restrict__ depth, const float* __restrict__ cam_view,
                                                                    const float* __restrict__ weight_in,
                                                                    const unsigned char* __restrict__ colors, float* __restrict__ tsdf,
                                                                    float* __restrict__ weight, float* __restrict__ color, TsdfGrid g,
                                                                    int xchunks, long tasks, int batch, int h, int w, float trunc,
                                                                    float max_weight, float min_depth, float max_depth) {
    // task = one wave's 64 consecutive i of one (j, k) row; four consecutive tasks per workgroup
    const long task = (long)blockIdx.x * (UM_TSDF_WG / 64) + (threadIdx.x >> 6);
    if (task >= tasks) return;
    const long row = task / xchunks;                           // j + ny k
    const int i = (int)(task - row * xchunks) * 64 + (threadIdx.x & 63);
    if (i >= g.nx) return;
    const int k = (int)(row / g.ny), j = (int)(row - (long)k * g.ny);
    const long vox = row * g.nx + i;
    const long planes = (long)g.nx * g.ny * g.nz;
    const float x = g.ox + (float)i * g.voxel, y = g.oy + (float)j * g.voxel, z = g.oz + (float)k * g.voxel;
    float T = tsdf[vox], W = weight[vox];
    float C0 = 0.f, C1 = 0.f, C2 = 0.f;
    if (color) {
        C0 = color[vox];
        C1 = color[planes + vox];
        C2 = color[2 * planes + vox];
    }
    const long L = (long)h * w;
    bool touched = false;
    for (int b = 0; b < batch; ++b) {
        const float* c = cam_view + (long)b * 30;
        const float X0 = c[9] * x + c[10] * y + c[11] * z + c[18];
        const float X1 = c[12] * x + c[13] * y + c[14] * z + c[19];
        const float X2 = c[15] * x + c[16] * y + c[17] * z + c[20];
        const float zz = c[27] * X0 + c[28] * X1 + c[29] * X2;
        // the skips come as early as they can: the launch is bound by arithmetic (two IEEE quotients to project, up to five to
        // update), and the 64 voxels of a wave mostly leave a view together
        if (!(zz > 1e-3f)) continue;                           // behind the camera (or NaN)
        const float u = (c[21] * X0 + c[22] * X1 + c[23] * X2) / zz;
        const float v = (c[24] * X0 + c[25] * X1 + c[26] * X2) / zz;
        const float px = rintf(u), py = rintf(v);
        // in view (false for a NaN position); the conversions below are then in range
        const bool in = px >= 0.f && px <= (float)(w - 1) && py >= 0.f && py <= (float)(h - 1);
        const long q = (long)b * L + (in ? (long)(int)py * w + (int)px : 0L);     // a clamped (in-frame) address; the tap is discarded
        if (!in) continue;
        const float d = depth[q];
        const float wi = weight_in ? weight_in[q] : 1.f;
        const float sdf = d - X2;
        const bool ok = tsdf_finite(d) && d > min_depth && d < max_depth && tsdf_finite(wi) && wi > 0.f && sdf >= -trunc;
        if (!ok) continue;
        const float f = fminf(1.f, sdf / trunc);
        const float Wn = W + wi;
        T = (T * W + f * wi) / Wn;
        if (color) {
            const unsigned char* cq = colors + q * 3;
            C0 = (C0 * W + (float)cq[0] * wi) / Wn;
            C1 = (C1 * W + (float)cq[1] * wi) / Wn;
            C2 = (C2 * W + (float)cq[2] * wi) / Wn;
        }
        W = fminf(Wn, max_weight);
        touched = true;
    }
    if (!touched) return;                                     // a voxel no view updated keeps its bytes
    tsdf[vox] = T;
    weight[vox] = W;
    if (color) {
        color[vox] = C0;
        color[planes + vox] = C1;
        color[2 * planes + vox] = C2;
    }
}

extern "C" int um_tsdf_integrate(const float* depth, const float* cam_view, const float* weight_in, const unsigned char* colors,
                                 float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* origin, float voxel,
                                 float trunc, float max_weight, float min_depth, float max_depth, int batch, int h, int w, void* stream) {
    if (!depth || !cam_view || !tsdf || !weight || !origin || (colors == nullptr) != (color == nullptr) || !tsdf_dims_ok(nx, ny, nz) ||
        batch <= 0 || h <= 0 || w <= 0 || (long)batch * h * w >= (1L << 31) || !tsdf_positive(voxel) || !tsdf_positive(trunc) ||
        !tsdf_positive(max_weight)) {
        um_set_error("um_tsdf_integrate: bad argument (dims=%d x %d x %d batch=%d h=%d w=%d voxel=%g trunc=%g max_weight=%g; "
                     "nx ny nz < 2^31; colors and color go together)", nx, ny, nz, batch, h, w, (double)voxel, (double)trunc,
                     (double)max_weight);
        return UM_ERR_BAD_ARG;
    }
    const TsdfGrid g = {nx, ny, nz, origin[0], origin[1], origin[2], voxel};
    const int xchunks = (nx + 63) / 64;
    const long tasks = (long)xchunks * ny * nz;
    const long blocks = (tasks + UM_TSDF_WG / 64 - 1) / (UM_TSDF_WG / 64);
    if (blocks >= (1L << 31)) {
        um_set_error("um_tsdf_integrate: bad argument (a %d x %d x %d volume needs %ld workgroups)", nx, ny, nz, blocks);
        return UM_ERR_BAD_ARG;
    }
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, (hipStream_t)stream);
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)blocks), dim3(UM_TSDF_WG), 0, (hipStream_t)stream, depth, cam_view,
                       weight_in, colors, tsdf, weight, color, g, xchunks, tasks, batch, h, w, trunc, max_weight, min_depth, max_depth);
    return (int)hipGetLastError();
}

// ---- surface points: stable compaction ------------------------------------------------------------------------------------------

// the crossings of voxel p along x, y, z as a bit mask (bit a = axis a), its coordinates and its value
__device__ __forceinline__ int tsdf_crossings(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g, long p,
                                              long total, float min_weight, int& i, int& j, int& k, float& tp, float tn[3]) {
    if (p >= total) return 0;
    const long row = p / g.nx;
    i = (int)(p - row * g.nx);
    k = (int)(row / g.ny);
    j = (int)(row - (long)k * g.ny);
    tp = tsdf[p];
    if (!(weight[p] >= min_weight) || !(fabsf(tp) < 1.f)) return 0;
    const bool inside[3] = {i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
    const long step[3] = {1L, (long)g.nx, (long)g.nx * g.ny};
    int m = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long n = inside[a] ? p + step[a] : p;           // a clamped (in-volume) address; the tap is discarded
        const float t = tsdf[n], wn = weight[n];
        tn[a] = t;
        if (inside[a] && wn >= min_weight && (tp < 0.f) != (t < 0.f) && fabsf(t) < 1.f) m |= 1 << a;
    }
    return m;
}

// phase 1: counts[workgroup] = number of crossings of the workgroup's 256 voxels
__global__ __launch_bounds__(UM_TSDF_WG) void tsdf_points_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                       int* __restrict__ counts, TsdfGrid g, long total,
                                                                       float min_weight) {
    __shared__ int wave_n[UM_TSDF_WG / 64];
    const long p = (long)blockIdx.x * UM_TSDF_WG + threadIdx.x;
    int i, j, k;
    float tp, tn[3];
    const int m = tsdf_crossings(tsdf, weight, g, p, total, min_weight, i, j, k, tp, tn);
    const int n = __popcll(__ballot(m & 1)) + __popcll(__ballot(m & 2)) + __popcll(__ballot(m & 4));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// phase 2: offsets[i] = counts[0] + ... + counts[i - 1], total[0] = the sum of all; one workgroup, each thread a contiguous run
__global__ __launch_bounds__(UM_TSDF_SCAN_WG) void tsdf_points_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                                           int* __restrict__ total, int n) {
    __shared__ int wave_sum[UM_TSDF_SCAN_WG / 64];
    const int per = (n + UM_TSDF_SCAN_WG - 1) / UM_TSDF_SCAN_WG;
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
    for (int q = 0; q < wave; ++q) before += wave_sum[q];
    int run = before + incl - s;
    for (long i = lo; i < hi; ++i) {
        const int c = counts[i];
        offsets[i] = run;
        run += c;
    }
    if (threadIdx.x == UM_TSDF_SCAN_WG - 1) total[0] = before + incl;
}

__device__ __forceinline__ unsigned char tsdf_byte(float v) {
    return (unsigned char)fminf(fmaxf(v == v ? rintf(v) : 0.f, 0.f), 255.f);
}

// phase 3: row (offset of the workgroup + rank inside it) of every crossing; rows >= capacity are not written
__global__ __launch_bounds__(UM_TSDF_WG) void tsdf_points_scatter_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                         const float* __restrict__ color, const int* __restrict__ offsets,
                                                                         float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                         TsdfGrid g, long total, float min_weight, int capacity) {
    __shared__ int wave_n[UM_TSDF_WG / 64];
    const long p = (long)blockIdx.x * UM_TSDF_WG + threadIdx.x;
    int i = 0, j = 0, k = 0;
    float tp = 0.f, tn[3] = {0.f, 0.f, 0.f};
    const int m = tsdf_crossings(tsdf, weight, g, p, total, min_weight, i, j, k, tp, tn);
    const unsigned long long m0 = __ballot(m & 1), m1 = __ballot(m & 2), m2 = __ballot(m & 4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(m0) + __popcll(m1) + __popcll(m2);
    __syncthreads();
    if (!m) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    int row = offsets[blockIdx.x] + __popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below);
    for (int q = 0; q < wave; ++q) row += wave_n[q];
    const float base[3] = {g.ox + (float)i * g.voxel, g.oy + (float)j * g.voxel, g.oz + (float)k * g.voxel};
    const long step[3] = {1L, (long)g.nx, (long)g.nx * g.ny};
    const long planes = (long)g.nx * g.ny * g.nz;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1 << a))) continue;
        if (row >= 0 && row < capacity) {
            const float s = tp / (tp - tn[a]);
            float* o = xyz + (long)row * 3;
            o[0] = a == 0 ? base[0] + s * g.voxel : base[0];
            o[1] = a == 1 ? base[1] + s * g.voxel : base[1];
            o[2] = a == 2 ? base[2] + s * g.voxel : base[2];
            if (rgb) {
                unsigned char* q = rgb + (long)row * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float cp = color[ch * planes + p], cn = color[ch * planes + p + step[a]];
                    q[ch] = tsdf_byte(cp + s * (cn - cp));
                }
            }
        }
        ++row;
    }
}

static inline long tsdf_point_groups(int nx, int ny, int nz) { return ((long)nx * ny * nz + UM_TSDF_WG - 1) / UM_TSDF_WG; }

extern "C" size_t um_tsdf_points_workspace_bytes(int nx, int ny, int nz) {
    if (!tsdf_dims_ok(nx, ny, nz)) return 0;
    return (size_t)tsdf_point_groups(nx, ny, nz) * 2 * sizeof(int);          // counts | offsets
}

extern "C" int um_tsdf_points(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const float* origin,
                              float voxel, float min_weight, float* xyz, unsigned char* rgb, int* count, int capacity, void* workspace,
                              size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tsdf || !weight || !origin || !xyz || !count || (color == nullptr) != (rgb == nullptr) || !tsdf_dims_ok(nx, ny, nz) ||
        capacity < 0 || !tsdf_positive(voxel) || min_weight != min_weight) {
        um_set_error("um_tsdf_points: bad argument (dims=%d x %d x %d capacity=%d voxel=%g min_weight=%g; nx ny nz < 2^31; color and rgb "
                     "go together)", nx, ny, nz, capacity, (double)voxel, (double)min_weight);
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_tsdf_points_workspace_bytes(nx, ny, nz);
    if (!workspace || ws_bytes < need || (uintptr_t)workspace % sizeof(int) != 0) {
        um_set_error("um_tsdf_points: workspace of %zu bytes, %zu needed (4-byte aligned)", ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const TsdfGrid g = {nx, ny, nz, origin[0], origin[1], origin[2], voxel};
    const long total = (long)nx * ny * nz;
    const int n = (int)tsdf_point_groups(nx, ny, nz);
    int* counts = (int*)workspace;
    int* offsets = counts + n;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(tsdf_points_count_kernel, dim3((unsigned)n), dim3(UM_TSDF_WG), 0, stream, tsdf, weight, counts, g, total,
                       min_weight);
    hipLaunchKernelGGL(tsdf_points_scan_kernel, dim3(1), dim3(UM_TSDF_SCAN_WG), 0, stream, (const int*)counts, offsets, count, n);
    hipLaunchKernelGGL(tsdf_points_scatter_kernel, dim3((unsigned)n), dim3(UM_TSDF_WG), 0, stream, tsdf, weight, color,
                       (const int*)offsets, xyz, rgb, g, total, min_weight, capacity);
    return (int)hipGetLastError();
}
