// Evaluation metrics of a batch of predictions, reduced on the device.                          gfx950 / wave64
//
//   um_flow_metrics   end-point error statistics of validate_sintel / validate_kitti (evaluate_flow.py:349-638): EPE, the 1 / 3 / 5 px
//                     shares, KITTI's F1 outliers, the three speed bins, matched / unmatched (compute_out_of_boundary_mask,
//                     utils/utils.py:79-103)
//   um_disp_metrics   loss/stereo_metric.py (epe, d1, thres 1 / 2 / 3, bad_pixel at its default thresholds) under the mask of
//                     evaluate_stereo.py (gt > 0, and gt < max_disp as validate_things)
//   um_depth_metrics  compute_errors (loss/depth_loss.py:6-24) under gt in (lo, hi) and valid
//
// The reference copies every prediction to the host (8 B/px over PCIe and a synchronisation per forward) and runs ~30 NumPy / ATen
// passes per sample.  Here every sample of the batch is read ONCE, in place: the padded prediction is indexed through the crop offset
// (top, left) of the InputPadder, never unpadded into a copy.  Per call two deterministic launches, like um_flow_to_rgb:
//
//   *_metrics_kernel   one thread per pixel, 8 pixels per thread (2048 per workgroup); float64 accumulators per thread, a wave folds by
//                      xor shuffles, the workgroup's four waves through LDS in wave order; one partial row [K] per workgroup into
//                      the workspace.  Every slot of the launch's geometry is rewritten each call: nothing of an earlier call is read.
//   metrics_fold_kernel  one workgroup per sample folds its partial rows in a fixed order (256 / K strided slices, then the slices in
//                      index order) into rows[b][K].
//
// No atomics, no arrival counters: the order of every addition is a function of the geometry alone, so rows are bitwise reproducible
// (and a sample's row does not depend on the batch it came in).  Counts are float64 (exact below 2^53).
//
// Per-pixel quantities are the reference's float32 values bit for bit: products and sums rounded separately (the file is compiled
// with -ffp-contract=off, build.py), correctly rounded square roots and divisions (met_sqrt, met_div below: epe / mag with mag == 0
// is inf or NaN as in the reference, a reciprocal would differ), float32 thresholds.  Only the accumulation is float64 where the
// reference pools float32 values pairwise.  The logarithms of the depth metrics are float64 logarithms of the float32 values.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

// IEEE square root and quotient.  NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define it as the native
// (1 ulp) square root, which differs from the IEEE one in the last bit for many inputs.  The plain operations are IEEE under
// -fhip-fp32-correctly-rounded-divide-sqrt, which build.py passes for this file explicitly (it is also hipcc's default).
__device__ __forceinline__ float met_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float met_div(float a, float b) { return a / b; }

#define UM_MET_PX 8                              // pixels per thread
#define UM_MET_CHUNK (256 * UM_MET_PX)           // pixels per workgroup = per partial row

// workgroup sum of K float64 accumulators per thread -> out[K] (written by threads 0..K-1); red: K * 4 doubles of LDS
template <int K>
__device__ __forceinline__ void block_fold(double (&acc)[K], double* red, double* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[k] = v;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = acc[k];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < K) out[t] = ((red[t] + red[K + t]) + red[2 * K + t]) + red[3 * K + t];
}

// rows[b][k] = the sum of sample b's partial rows, in an order that depends on (chunks, K) only
template <int K>
__global__ __launch_bounds__(256) void metrics_fold_kernel(const double* __restrict__ partial, double* __restrict__ rows, int chunks) {
    constexpr int S = 256 / K;
    __shared__ double red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int k = t % K, s = t / K;
    const double* p = partial + (long)b * chunks * K;
    double v = 0.0;
    for (int i = s; i < chunks; i += S) v += p[(long)i * K + k];
    red[t] = v;                                    // t == s * K + k
    __syncthreads();
    if (t < K) {
        double r = red[t];
#pragma unroll
        for (int j = 1; j < S; ++j) r += red[j * K + t];
        rows[(long)b * K + t] = r;
    }
}

// ---- optical flow ---------------------------------------------------------------------------------------------------------------
// row: 0 n | 1 sum epe | 2 3 4 n(epe > 1, 3, 5) | 5 n(outlier) | 6 7 n, sum (mag < 10) | 8 9 (10 <= mag <= 40) | 10 11 (mag > 40) |
//      12 13 n, sum matched | 14 15 n, sum unmatched
__global__ __launch_bounds__(256) void flow_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const float* __restrict__ valid, const float* __restrict__ noc,
                                                           double* __restrict__ partial, int hp, int wp, int h, int w, int top,
                                                           int left, int chunks) {
    constexpr int K = UM_FLOW_METRICS_K;
    __shared__ double red[4 * K];
    const int b = blockIdx.y;
    const int L = h * w;
    const long Lp = (long)hp * wp;
    const float* gu = gt + (long)b * 2 * L;
    const float* gv = gu + L;
    const float* pu = pred + (long)b * 2 * Lp;
    const float* pv = pu + Lp;
    const float* va = valid ? valid + (long)b * L : nullptr;
    const float* nv = noc ? noc + (long)b * L : nullptr;
    const float wmax = (float)(w - 1), hmax = (float)(h - 1);
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int base = blockIdx.x * UM_MET_CHUNK + threadIdx.x;
#pragma unroll
    for (int i = 0; i < UM_MET_PX; ++i) {
        const int p = base + i * 256;
        if (p < L) {
            const int y = p / w, x = p - y * w;
            const long q = (long)(y + top) * wp + (x + left);
            const float u = gu[p], v = gv[p];
            const float du = pu[q] - u, dv = pv[q] - v;
            const float epe = met_sqrt(du * du + dv * dv);
            const float mag = met_sqrt(u * u + v * v);
            const bool m = va ? va[p] >= 0.5f : true;
            const double e = (double)epe;
            acc[0] += m ? 1.0 : 0.0;
            acc[1] += m ? e : 0.0;
            acc[2] += (m && epe > 1.0f) ? 1.0 : 0.0;
            acc[3] += (m && epe > 3.0f) ? 1.0 : 0.0;
            acc[4] += (m && epe > 5.0f) ? 1.0 : 0.0;
            acc[5] += (m && epe > 3.0f && met_div(epe, mag) > 0.05f) ? 1.0 : 0.0;
            const bool s0 = m && mag < 10.0f, s1 = m && mag >= 10.0f && mag <= 40.0f, s2 = m && mag > 40.0f;
            acc[6] += s0 ? 1.0 : 0.0;
            acc[7] += s0 ? e : 0.0;
            acc[8] += s1 ? 1.0 : 0.0;
            acc[9] += s1 ? e : 0.0;
            acc[10] += s2 ? 1.0 : 0.0;
            acc[11] += s2 ? e : 0.0;
            if (nv) {
                // the ground-truth target stays in frame: coords + flow in float32, as compute_out_of_boundary_mask forms it
                const float cx = (float)x + u, cy = (float)y + v;
                const bool inframe = cx >= 0.0f && cx <= wmax && cy >= 0.0f && cy <= hmax && fabsf(u) <= wmax && fabsf(v) <= hmax;
                const bool mt = nv[p] > 0.5f && inframe;
                acc[12] += (m && mt) ? 1.0 : 0.0;
                acc[13] += (m && mt) ? e : 0.0;
                acc[14] += (m && !mt) ? 1.0 : 0.0;
                acc[15] += (m && !mt) ? e : 0.0;
            }
        }
    }
    block_fold<K>(acc, red, partial + ((long)b * chunks + blockIdx.x) * K);
}

// ---- disparity ------------------------------------------------------------------------------------------------------------------
// row: 0 n | 1 sum |est - gt| | 2 3 4 n(e > 1, 2, 3) | 5 n(d1) | 6 n(bad pixel: e > 10 and e / max(gt, 1) > 0.1) | 7 unused (0)
__global__ __launch_bounds__(256) void disp_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           double* __restrict__ partial, int hp, int wp, int h, int w, int top,
                                                           int left, float max_disp, int chunks) {
    constexpr int K = UM_DISP_METRICS_K;
    __shared__ double red[4 * K];
    const int b = blockIdx.y;
    const int L = h * w;
    const float* g = gt + (long)b * L;
    const float* pr = pred + (long)b * hp * wp;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int base = blockIdx.x * UM_MET_CHUNK + threadIdx.x;
#pragma unroll
    for (int i = 0; i < UM_MET_PX; ++i) {
        const int p = base + i * 256;
        if (p < L) {
            const int y = p / w, x = p - y * w;
            const float d = g[p], est = pr[(long)(y + top) * wp + (x + left)];
            const bool m = d > 0.0f && (max_disp > 0.0f ? d < max_disp : true);
            const float e = fabsf(d - est);
            acc[0] += m ? 1.0 : 0.0;
            acc[1] += m ? (double)e : 0.0;
            acc[2] += (m && e > 1.0f) ? 1.0 : 0.0;
            acc[3] += (m && e > 2.0f) ? 1.0 : 0.0;
            acc[4] += (m && e > 3.0f) ? 1.0 : 0.0;
            acc[5] += (m && e > 3.0f && met_div(e, d) > 0.05f) ? 1.0 : 0.0;
            acc[6] += (m && e > 10.0f && met_div(e, fmaxf(d, 1.0f)) > 0.1f) ? 1.0 : 0.0;
        }
    }
    block_fold<K>(acc, red, partial + ((long)b * chunks + blockIdx.x) * K);
}

// ---- depth ----------------------------------------------------------------------------------------------------------------------
// row: 0 n | 1 sum |gt - pred| / gt | 2 sum (gt - pred)^2 / gt | 3 sum (gt - pred)^2 | 4 sum (ln gt - ln pred)^2 |
//      5 6 7 n(max(gt / pred, pred / gt) < 1.25, 1.25^2, 1.25^3)          (1.5625 and 1.953125 are exact in float32)
__global__ __launch_bounds__(256) void depth_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                            const float* __restrict__ valid, double* __restrict__ partial, int hp,
                                                            int wp, int h, int w, int top, int left, float lo, float hi, int chunks) {
    constexpr int K = UM_DEPTH_METRICS_K;
    __shared__ double red[4 * K];
    const int b = blockIdx.y;
    const int L = h * w;
    const float* g = gt + (long)b * L;
    const float* pr = pred + (long)b * hp * wp;
    const float* va = valid ? valid + (long)b * L : nullptr;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int base = blockIdx.x * UM_MET_CHUNK + threadIdx.x;
#pragma unroll
    for (int i = 0; i < UM_MET_PX; ++i) {
        const int p = base + i * 256;
        if (p < L) {
            const int y = p / w, x = p - y * w;
            const float d = g[p], est = pr[(long)(y + top) * wp + (x + left)];
            const bool m = d > lo && d < hi && (va ? va[p] > 0.5f : true);
            const float r0 = met_div(d, est), r1 = met_div(est, d);
            // np.maximum propagates a NaN (every comparison with it is false); fmaxf would drop it
            const float th = (r0 != r0 || r1 != r1) ? __builtin_nanf("") : fmaxf(r0, r1);
            const float diff = d - est;
            const float sq = diff * diff;
            const double dl = log((double)d) - log((double)est);
            acc[0] += m ? 1.0 : 0.0;
            acc[1] += m ? (double)met_div(fabsf(diff), d) : 0.0;
            acc[2] += m ? (double)met_div(sq, d) : 0.0;
            acc[3] += m ? (double)sq : 0.0;
            acc[4] += m ? dl * dl : 0.0;
            acc[5] += (m && th < 1.25f) ? 1.0 : 0.0;
            acc[6] += (m && th < 1.5625f) ? 1.0 : 0.0;
            acc[7] += (m && th < 1.953125f) ? 1.0 : 0.0;
        }
    }
    block_fold<K>(acc, red, partial + ((long)b * chunks + blockIdx.x) * K);
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
static inline bool met_size_ok(int batch, int h, int w) {
    return batch > 0 && batch <= 65535 && h > 0 && w > 0 && (long)h * w <= (1L << 30);
}

static inline bool met_crop_ok(int hp, int wp, int h, int w, int top, int left) {
    return hp > 0 && wp > 0 && (long)hp * wp <= (1L << 30) && top >= 0 && left >= 0 && (long)top + h <= hp && (long)left + w <= wp;
}

static inline int met_chunks(int h, int w) { return (int)(((long)h * w + UM_MET_CHUNK - 1) / UM_MET_CHUNK); }

static inline size_t met_ws_bytes(int batch, int h, int w, int k) {
    if (!met_size_ok(batch, h, w)) return 0;
    return (size_t)batch * (size_t)met_chunks(h, w) * (size_t)k * sizeof(double);
}

// the checks every entry point shares; 0 when the call may launch
static int met_check(const char* name, bool pointers, int batch, int hp, int wp, int h, int w, int top, int left, const void* workspace,
                     size_t ws_bytes, size_t need) {
    if (!pointers || !met_size_ok(batch, h, w)) {
        um_set_error("%s: bad argument (batch=%d h=%d w=%d)", name, batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    if (!met_crop_ok(hp, wp, h, w, top, left)) {
        um_set_error("%s: the crop %dx%d at (%d, %d) leaves the padded frame %dx%d", name, h, w, top, left, hp, wp);
        return UM_ERR_BAD_ARG;
    }
    if (!workspace || ws_bytes < need || ((uintptr_t)workspace & 7)) {
        um_set_error("%s: workspace of %zu bytes (8-byte aligned), %zu needed", name, ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    return 0;
}

extern "C" size_t um_flow_metrics_workspace_bytes(int batch, int h, int w) { return met_ws_bytes(batch, h, w, UM_FLOW_METRICS_K); }
extern "C" size_t um_disp_metrics_workspace_bytes(int batch, int h, int w) { return met_ws_bytes(batch, h, w, UM_DISP_METRICS_K); }
extern "C" size_t um_depth_metrics_workspace_bytes(int batch, int h, int w) { return met_ws_bytes(batch, h, w, UM_DEPTH_METRICS_K); }

extern "C" int um_flow_metrics(const float* pred, const float* gt, const float* valid, const float* noc_valid, double* rows, int batch,
                               int hp, int wp, int h, int w, int top, int left, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int err = met_check("um_flow_metrics", pred && gt && rows, batch, hp, wp, h, w, top, left, workspace, ws_bytes,
                              um_flow_metrics_workspace_bytes(batch, h, w));
    if (err) return err;
    const int chunks = met_chunks(h, w);
    double* partial = (double*)workspace;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(flow_metrics_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(256), 0, stream, pred, gt, valid, noc_valid,
                       partial, hp, wp, h, w, top, left, chunks);
    hipLaunchKernelGGL(metrics_fold_kernel<UM_FLOW_METRICS_K>, dim3((unsigned)batch), dim3(256), 0, stream, (const double*)partial, rows,
                       chunks);
    return (int)hipGetLastError();
}

extern "C" int um_disp_metrics(const float* pred, const float* gt, double* rows, int batch, int hp, int wp, int h, int w, int top,
                               int left, float max_disp, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int err = met_check("um_disp_metrics", pred && gt && rows, batch, hp, wp, h, w, top, left, workspace, ws_bytes,
                              um_disp_metrics_workspace_bytes(batch, h, w));
    if (err) return err;
    const int chunks = met_chunks(h, w);
    double* partial = (double*)workspace;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(disp_metrics_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(256), 0, stream, pred, gt, partial, hp, wp, h,
                       w, top, left, max_disp, chunks);
    hipLaunchKernelGGL(metrics_fold_kernel<UM_DISP_METRICS_K>, dim3((unsigned)batch), dim3(256), 0, stream, (const double*)partial, rows,
                       chunks);
    return (int)hipGetLastError();
}

extern "C" int um_depth_metrics(const float* pred, const float* gt, const float* valid, double* rows, int batch, int hp, int wp, int h,
                                int w, int top, int left, float lo, float hi, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int err = met_check("um_depth_metrics", pred && gt && rows, batch, hp, wp, h, w, top, left, workspace, ws_bytes,
                              um_depth_metrics_workspace_bytes(batch, h, w));
    if (err) return err;
    const int chunks = met_chunks(h, w);
    double* partial = (double*)workspace;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(depth_metrics_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(256), 0, stream, pred, gt, valid, partial, hp,
                       wp, h, w, top, left, lo, hi, chunks);
    hipLaunchKernelGGL(metrics_fold_kernel<UM_DEPTH_METRICS_K>, dim3((unsigned)batch), dim3(256), 0, stream, (const double*)partial, rows,
                       chunks);
    return (int)hipGetLastError();
}
