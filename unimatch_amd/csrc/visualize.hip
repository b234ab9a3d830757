// Scalar map -> colour image: the reference's vis_disparity and viz_depth_tensor (utils/visualization.py:11-16, 92-107) per image of a
// batch, on the device.                                                                                          gfx950 / wave64
//
//   um_scalar_to_rgb   x [B,h,w] fp32 -> rgb [B,h,w,3] uint8 through a 256-entry table.  v = x or 1 / x; per image vmin = min v and
//                      vmax = max v (UM_NORM_MINMAX_255) or the 95th percentile of v with linear interpolation between the two
//                      neighbouring order statistics (UM_NORM_MIN_P95_256); idx from ((v - vmin) / (vmax - vmin)) * 255 or * 256.
//
// The order statistics are a radix select per image over order-preserving 32-bit keys of the fp32 values (sign bit flipped for
// positive values, all bits for negative ones), three digits of 11, 11 and 10 bits, most significant first.  Ranks lo and hi = lo + 1
// are selected together: each carries its own key prefix, and while the prefixes are equal one histogram serves both.  A pass is two
// launches:
//   vis_hist_kernel    a workgroup counts the digit of the keys of its 16384 pixels that match a rank's prefix in an LDS histogram
//                      (LDS atomics only) and writes the whole histogram into its own workspace slot; pass 0 also writes the
//                      workgroup's minimum and maximum.
//   vis_fold_kernel    one workgroup per image sums the slots in index order, scans the bins, and writes the digit that holds each
//                      rank and the rank inside that digit into the image's state record; the last pass turns the two keys back into
//                      floats and interpolates vmax in float64.
// then vis_colour_kernel reads (vmin, vmax) and colours.  No global atomics, no arrival counters; every workspace slot a launch reads
// was written earlier by the same call (histogram slots of rank hi are neither written nor read while the prefixes are equal), so
// nothing depends on a zeroed or left-over workspace and two calls give equal bits.  The selected values are elements of the input
// for any distribution: after three digits the whole key is known.  UM_NORM_MINMAX_255 runs pass 0 without a histogram.
//
// LDS: two histograms of 2048 counters = 16 KiB per workgroup of 256 threads, which leaves the CU's 160 KiB room for eight
// workgroups: the register file, not the LDS, bounds the occupancy.
//
// All value arithmetic is fp32 with separately rounded operations and IEEE division (-ffp-contract=off,
// -fhip-fp32-correctly-rounded-divide-sqrt in build.py), so the host restatement (unimatch_amd/visualize.py) gives the same bits.
// NaN / infinite inputs are outside the reference contract: the kernels terminate and stay in bounds (keys of NaNs sort beyond the
// infinities, minima and maxima skip NaNs), and a pixel whose normalised value is NaN gets index 0.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

#define UM_VIS_THREADS 256
#define UM_VIS_PX 64                                  // pixels per thread of a histogram launch
#define UM_VIS_CHUNK (UM_VIS_THREADS * UM_VIS_PX)     // 16384 pixels per workgroup
#define UM_VIS_BINS 2048                              // the widest digit: 11 bits
#define UM_VIS_COLOUR_PX 4                            // pixels per thread of the colour launch (12 bytes: three 4-byte stores)

struct VisState {                                     // one per image, in the workspace
    unsigned prefix[2];                               // the key bits found so far of ranks lo, hi (right-aligned)
    unsigned rank[2];                                 // the ranks inside the elements that share the prefix
    float vmin, vmax;
    unsigned pad[2];
};

__device__ __forceinline__ unsigned vis_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float vis_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float vis_value(float x, int inverse) { return inverse ? 1.0f / x : x; }

// workspace layout: VisState[B] | float mm[B][chunks][2] | unsigned hist[B][chunks][2][UM_VIS_BINS]
struct VisWs {
    VisState* state;
    float* mm;
    unsigned* hist;
};

static inline size_t vis_align(size_t n) { return (n + 255) & ~(size_t)255; }

static inline VisWs vis_carve(void* ws, int batch, int chunks) {
    char* p = (char*)ws;
    VisWs r;
    r.state = (VisState*)p;
    p += vis_align((size_t)batch * sizeof(VisState));
    r.mm = (float*)p;
    p += vis_align((size_t)batch * chunks * 2 * sizeof(float));
    r.hist = (unsigned*)p;
    return r;
}

// ---- histogram of one digit ------------------------------------------------------------------------------------------------------
// PASS 0: digit = key >> 21, every key matches, min / max ride along.  PASS 1: keys with key >> 21 == prefix, digit (key >> 10) & 2047.
// PASS 2: keys with key >> 10 == prefix, digit key & 1023.  HIST = false (min-max normalisation): pass 0 without the histogram.
template <int PASS, bool HIST>
__global__ __launch_bounds__(UM_VIS_THREADS) void vis_hist_kernel(const float* __restrict__ x, VisWs ws, int L, int chunks, int inverse) {
    __shared__ unsigned hist[2][UM_VIS_BINS];
    __shared__ float red[2][UM_VIS_THREADS / 64];
    constexpr int BINS = PASS == 2 ? 1024 : 2048;
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (long)b * L;
    unsigned p0 = 0, p1 = 0;
    if (PASS > 0) {
        p0 = ws.state[b].prefix[0];
        p1 = ws.state[b].prefix[1];
    }
    const bool same = p0 == p1;
    if (HIST) {
        for (int i = tid; i < (same ? BINS : 2 * BINS); i += UM_VIS_THREADS) hist[i / BINS][i % BINS] = 0;
        __syncthreads();
    }
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const int base = chunk * UM_VIS_CHUNK + tid;
#pragma unroll 8
    for (int i = 0; i < UM_VIS_PX; ++i) {
        const int p = base + i * UM_VIS_THREADS;
        if (p < L) {
            const float v = vis_value(xb[p], inverse);
            if (PASS == 0) {
                lo = fminf(lo, v);                    // (fminf / fmaxf skip NaNs)
                hi = fmaxf(hi, v);
            }
            if (HIST) {
                const unsigned k = vis_key(v);
                if (PASS == 0) {
                    atomicAdd(&hist[0][k >> 21], 1u);
                } else {
                    const unsigned head = PASS == 1 ? k >> 21 : k >> 10;
                    const unsigned digit = PASS == 1 ? (k >> 10) & 2047u : k & 1023u;
                    if (head == p0) atomicAdd(&hist[0][digit], 1u);
                    if (!same && head == p1) atomicAdd(&hist[1][digit], 1u);
                }
            }
        }
    }
    if (PASS == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = lo;
            red[1][tid >> 6] = hi;
        }
    }
    __syncthreads();
    if (PASS == 0 && tid == 0) {
        float* mm = ws.mm + ((long)b * chunks + chunk) * 2;
        mm[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        mm[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
    if (HIST) {
        unsigned* out = ws.hist + ((long)b * chunks + chunk) * 2 * UM_VIS_BINS;
        for (int i = tid; i < BINS; i += UM_VIS_THREADS) out[i] = hist[0][i];
        if (!same)
            for (int i = tid; i < BINS; i += UM_VIS_THREADS) out[UM_VIS_BINS + i] = hist[1][i];
    }
}

// ---- fold: the digit that holds each rank -------------------------------------------------------------------------------------------
// One workgroup per image.  rank_lo / rank_hi: the ranks of the whole image (read in pass 0; later passes read the state record).
// LAST: the keys are complete -> vmax = (float)(a_lo + (a_hi - a_lo) * t) in float64, stats_out.  nbins == 0: min-max mode, no select.
__global__ __launch_bounds__(UM_VIS_THREADS) void vis_fold_kernel(VisWs ws, int chunks, int pass, int nbins, int bits, int last,
                                                                  unsigned rank_lo, unsigned rank_hi, double t, float* stats_out) {
    __shared__ unsigned cnt[2][UM_VIS_BINS];
    __shared__ unsigned tsum[2][UM_VIS_THREADS];
    __shared__ float red[2][UM_VIS_THREADS / 64];
    __shared__ unsigned found[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    VisState* st = ws.state + b;
    if (pass == 0) {                                  // the image's minimum and maximum, partials in index order
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int c = tid; c < chunks; c += UM_VIS_THREADS) {
            lo = fminf(lo, ws.mm[((long)b * chunks + c) * 2]);
            hi = fmaxf(hi, ws.mm[((long)b * chunks + c) * 2 + 1]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = lo;
            red[1][tid >> 6] = hi;
        }
        __syncthreads();
        if (tid == 0) {
            lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
            hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
            st->vmin = lo;
            st->vmax = hi;                            // (replaced by the percentile after the last pass)
            if (nbins == 0 && stats_out) {
                stats_out[2 * b] = lo;
                stats_out[2 * b + 1] = hi;
            }
        }
        if (nbins == 0) return;
    }
    unsigned p0 = 0, p1 = 0, r0 = rank_lo, r1 = rank_hi;
    if (pass > 0) {
        p0 = st->prefix[0];
        p1 = st->prefix[1];
        r0 = st->rank[0];
        r1 = st->rank[1];
    }
    const bool same = p0 == p1;
    const unsigned* part = ws.hist + (long)b * chunks * 2 * UM_VIS_BINS;
    for (int bin = tid; bin < nbins; bin += UM_VIS_THREADS) {
        unsigned s0 = 0, s1 = 0;
        for (int c = 0; c < chunks; ++c) {
            s0 += part[(long)c * 2 * UM_VIS_BINS + bin];
            if (!same) s1 += part[(long)c * 2 * UM_VIS_BINS + UM_VIS_BINS + bin];
        }
        cnt[0][bin] = s0;
        cnt[1][bin] = same ? s0 : s1;
    }
    __syncthreads();
    const int per = nbins / UM_VIS_THREADS;           // 8 or 4 consecutive bins per thread
    unsigned own[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        unsigned s = 0;
        for (int j = 0; j < per; ++j) s += cnt[g][tid * per + j];
        own[g] = s;
        tsum[g][tid] = s;
    }
    __syncthreads();
    for (int off = 1; off < UM_VIS_THREADS; off <<= 1) {          // inclusive scan of the threads' sums
        const unsigned a0 = tid >= off ? tsum[0][tid - off] : 0u, a1 = tid >= off ? tsum[1][tid - off] : 0u;
        __syncthreads();
        tsum[0][tid] += a0;
        tsum[1][tid] += a1;
        __syncthreads();
    }
    const unsigned total[2] = {tsum[0][UM_VIS_THREADS - 1], tsum[1][UM_VIS_THREADS - 1]};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        unsigned r = g == 0 ? r0 : r1;
        // a rank is always below the count of its prefix; the clamp only keeps a corrupted state inside the table
        if (total[g] > 0 && r >= total[g]) r = total[g] - 1;
        unsigned before = tsum[g][tid] - own[g];
        if (own[g] > 0 && r >= before && r < before + own[g]) {   // exactly one thread
            int bin = tid * per;
            for (int j = 0; j < per; ++j, ++bin) {
                const unsigned c = cnt[g][bin];
                if (r < before + c) break;
                before += c;
            }
            bin = min(bin, nbins - 1);
            const unsigned p = g == 0 ? p0 : p1;
            found[g] = pass == 0 ? (unsigned)bin : ((p << bits) | (unsigned)bin);
            st->prefix[g] = found[g];
            st->rank[g] = r - before;
        }
    }
    if (!last) return;
    __syncthreads();
    if (tid == 0) {
        const float alo = vis_unkey(found[0]), ahi = vis_unkey(found[1]);
        const float vmax = (float)((double)alo + ((double)ahi - (double)alo) * t);
        st->vmax = vmax;
        if (stats_out) {
            stats_out[2 * b] = st->vmin;
            stats_out[2 * b + 1] = vmax;
        }
    }
}

// ---- colour --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int vis_index(float x, int inverse, int norm, float vmin, float vmax) {
    const float v = vis_value(x, inverse);
    const float q = (v - vmin) / (vmax - vmin);
    if (norm == UM_NORM_MINMAX_255) {
        const float xa = q * 255.0f;
        return xa != xa ? 0 : (int)fminf(fmaxf(xa, 0.0f), 255.0f);
    }
    if (vmax == vmin) return 0;
    const float xa = q * 256.0f;
    if (xa != xa) return 0;
    return xa >= 256.0f ? 255 : (int)fminf(fmaxf(xa, 0.0f), 255.0f);
}

__global__ __launch_bounds__(UM_VIS_THREADS) void vis_colour_kernel(const float* __restrict__ x, const VisState* __restrict__ state,
                                                                    const unsigned char* __restrict__ lut, unsigned char* __restrict__ rgb,
                                                                    int L, int inverse, int norm, int vec) {
    __shared__ unsigned char table[256 * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 256 * 3; i += UM_VIS_THREADS) table[i] = lut[i];
    __syncthreads();
    const float vmin = state[b].vmin, vmax = state[b].vmax;
    const float* xb = x + (long)b * L;
    unsigned char* ob = rgb + (long)b * L * 3;
    const int p0 = (blockIdx.x * UM_VIS_THREADS + tid) * UM_VIS_COLOUR_PX;
    if (p0 >= L) return;
    if (vec && p0 + UM_VIS_COLOUR_PX <= L) {
        // vec (host): L % 4 == 0, x 16-byte and rgb 4-byte aligned, so every image's plane is 16-byte aligned and its bytes start at
        // a multiple of 12
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xb + p0);
        unsigned char px[UM_VIS_COLOUR_PX * 3];
#pragma unroll
        for (int i = 0; i < UM_VIS_COLOUR_PX; ++i) {
            const int idx = vis_index(x4[i], inverse, norm, vmin, vmax);
            px[3 * i] = table[3 * idx];
            px[3 * i + 1] = table[3 * idx + 1];
            px[3 * i + 2] = table[3 * idx + 2];
        }
        unsigned* dst = reinterpret_cast<unsigned*>(ob + (long)p0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dst[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
        return;
    }
    for (int i = 0; i < UM_VIS_COLOUR_PX && p0 + i < L; ++i) {
        const int idx = vis_index(xb[p0 + i], inverse, norm, vmin, vmax);
        ob[(long)(p0 + i) * 3] = table[3 * idx];
        ob[(long)(p0 + i) * 3 + 1] = table[3 * idx + 1];
        ob[(long)(p0 + i) * 3 + 2] = table[3 * idx + 2];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static inline bool vis_args_ok(int batch, int h, int w) {
    return batch > 0 && batch <= 65535 && h > 0 && w > 0 && (long)h * w <= (1L << 30);
}

extern "C" size_t um_scalar_to_rgb_workspace_bytes(int batch, int h, int w) {
    if (!vis_args_ok(batch, h, w)) return 0;
    const size_t chunks = (size_t)(((long)h * w + UM_VIS_CHUNK - 1) / UM_VIS_CHUNK);
    const size_t slots = chunks;
    return vis_align((size_t)batch * sizeof(VisState)) + vis_align((size_t)batch * chunks * 2 * sizeof(float)) +
           (size_t)batch * slots * 2 * UM_VIS_BINS * sizeof(unsigned);
}

extern "C" int um_scalar_to_rgb(const float* x, unsigned char* rgb, int batch, int h, int w, int inverse, int norm,
                                const unsigned char* lut, float* stats_out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !rgb || !lut || !vis_args_ok(batch, h, w) || (norm != UM_NORM_MINMAX_255 && norm != UM_NORM_MIN_P95_256)) {
        um_set_error("um_scalar_to_rgb: bad argument (batch=%d h=%d w=%d norm=%d)", batch, h, w, norm);
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_scalar_to_rgb_workspace_bytes(batch, h, w);
    if (!workspace || ws_bytes < need || (uintptr_t)workspace % 8 != 0) {
        um_set_error("um_scalar_to_rgb: workspace of %zu bytes (8-byte aligned), %zu needed", ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const int L = h * w, inv = inverse ? 1 : 0;
    const int chunks = (L + UM_VIS_CHUNK - 1) / UM_VIS_CHUNK;
    const VisWs ws = vis_carve(workspace, batch, chunks);
    const dim3 hgrid((unsigned)chunks, (unsigned)batch), fgrid((unsigned)batch), block(UM_VIS_THREADS);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    if (norm == UM_NORM_MINMAX_255) {
        hipLaunchKernelGGL((vis_hist_kernel<0, false>), hgrid, block, 0, stream, x, ws, L, chunks, inv);
        hipLaunchKernelGGL(vis_fold_kernel, fgrid, block, 0, stream, ws, chunks, 0, 0, 0, 0, 0u, 0u, 0.0, stats_out);
    } else {
        // np.percentile(v, 95), linear: k = 0.95 (n - 1) in float64, between the order statistics floor(k) and floor(k) + 1
        const double k = 0.95 * (double)(L - 1);
        const long lo = (long)k;                      // k >= 0: truncation is the floor
        const long hi = lo + 1 < L ? lo + 1 : L - 1;
        const double t = k - (double)lo;
        hipLaunchKernelGGL((vis_hist_kernel<0, true>), hgrid, block, 0, stream, x, ws, L, chunks, inv);
        hipLaunchKernelGGL(vis_fold_kernel, fgrid, block, 0, stream, ws, chunks, 0, 2048, 11, 0, (unsigned)lo, (unsigned)hi, t, stats_out);
        hipLaunchKernelGGL((vis_hist_kernel<1, true>), hgrid, block, 0, stream, x, ws, L, chunks, inv);
        hipLaunchKernelGGL(vis_fold_kernel, fgrid, block, 0, stream, ws, chunks, 1, 2048, 11, 0, 0u, 0u, t, stats_out);
        hipLaunchKernelGGL((vis_hist_kernel<2, true>), hgrid, block, 0, stream, x, ws, L, chunks, inv);
        hipLaunchKernelGGL(vis_fold_kernel, fgrid, block, 0, stream, ws, chunks, 2, 1024, 10, 1, 0u, 0u, t, stats_out);
    }
    const int groups = (L + UM_VIS_THREADS * UM_VIS_COLOUR_PX - 1) / (UM_VIS_THREADS * UM_VIS_COLOUR_PX);
    const int vec = (L % 4 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)rgb % 4 == 0);
    hipLaunchKernelGGL(vis_colour_kernel, dim3((unsigned)groups, (unsigned)batch), block, 0, stream, x, (const VisState*)ws.state, lut,
                       rgb, L, inv, norm, vec);
    return (int)hipGetLastError();
}
