// Matching confidence: statistics of every row of the global matching distribution, fused.     gfx950 / wave64 / MFMA
//
//   p_ij = softmax_j( q_i . k_j / sqrt(C) )         the `prob` the reference's global_correlation_softmax (unimatch/matching.py:7-36)
//                                                   and global_correlation_softmax_stereo (matching.py:126-151) return next to the flow
//   max_prob_i = max_j p_ij      best_i = argmax_j p_ij (lowest index on a tie)      entropy_i = -sum_j p_ij ln p_ij
//   mean_i = sum_j p_ij (g_j - g_i)                 variance_i = sum_j p_ij |g_j - g_i - mean_i|^2          (g = pixel coordinates)
//
// The L x L matrix is never formed (that is what the fused kernels of global_match.hip are for); a caller who wanted these had to
// rebuild it in torch.  match_stats_kernel borrows gsv3_kernel's geometry -- operand planes carrying sqrt(log2(e) / sqrt(C)) on both
// sides (scores arrive in log2 units), S^T = K . Q^T with v_mfma_f32_32x32x16, a lane owns one query and 16 of the 32 keys of a
// sub-tile, the two half-waves of a query keep independent states merged once at the end, 64-key tiles through LDS-DMA, ragged and
// causal masking -- but NOT its instruction-level interleave: this is an optional path, a tile's MFMAs and its softmax terms are two
// plain phases and the compiler schedules them.  gsv3_kernel / gsv4_kernel are untouched.
//
// Running state of a lane (MsState), one pass over the keys:
//   M    integer offset, ceil of the running maximum: p = 2^(s - M) <= 1, and every rescale factor 2^-(M' - M) is an exact power of two
//   mt   the running maximum itself, j its key (the lowest such key)
//   l    sum 2^(s - M)
//   e    sum 2^(s - M) (s - mt)     relative to the TRUE maximum: the best key's own term is exactly 0, so a row with one key gives
//                                   entropy = ln(l / 2^(mt - M)) - ln2 e / l = ln 1 - 0 = 0 exactly; when mt rises by d: e -= d l
//   sx, sy, srr   sum 2^(s - M) dx, dy, dx^2 + dy^2 with (dx, dy) = g_j - g_i taken relative to the lane's OWN query pixel, so that
//                 the cancellation in E|d|^2 - |E d|^2 is bounded by the flow magnitude and not by the map size
// ms_merge() combines two partial states; it is written once and serves the half-wave merge (and would serve a key split).
// Stereo: every scanline is a launch row ("batch" entry) of w tokens on a 1-row grid (y == 0 everywhere), keys x' <= x.
//
// Memory contract: reads the two feature tensors (through the planes in the caller's workspace), writes every element of stats,
// best and mean (when given) and nothing else; the workspace holds the planes only.
#include "common.h"
#include "planes.h"

struct MsArgs {
    const unsigned short* qp;   // [NS][nbatch][Lq][128]
    const unsigned short* kp;   // [NS][nbatch][Lk][128]
    long q_plane_stride, k_plane_stride;
    float* stats;               // [images][3][rows * Lq]
    int* best;                  // [images][rows * Lq]
    float* mean;                // [images][nmean][rows * Lq] or nullptr
    int Lq, Lk;
    int gw;                     // width of the pixel grid a token index lives on (flow: w; stereo: the scanline itself)
    int rows;                   // launch rows per image (flow: 1; stereo: h)
    int nmean;                  // channels of `mean` (flow: 2; stereo: 1)
};

struct MsState {
    float M, mt;
    int j;
    float l, e, sx, sy, srr;
};

__device__ __forceinline__ MsState ms_empty() { return MsState{UM_NEG_INIT, UM_NEG_INIT, 0x7fffffff, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// Two partial states of one query over disjoint key sets -> the state over their union.  An empty side (l == 0, M == mt ==
// UM_NEG_INIT) contributes factor 2^-1e30 == 0 and 0 * finite corrections.
__device__ __forceinline__ MsState ms_merge(const MsState& a, const MsState& b) {
    MsState r;
    const bool bw = (b.mt > a.mt) || (b.mt == a.mt && b.j < a.j);
    r.mt = bw ? b.mt : a.mt;
    r.j = bw ? b.j : a.j;
    r.M = fmaxf(a.M, b.M);
    const float fa = fast_exp2(a.M - r.M), fb = fast_exp2(b.M - r.M);
    const float ea = a.e - (r.mt - a.mt) * a.l, eb = b.e - (r.mt - b.mt) * b.l;
    r.l = a.l * fa + b.l * fb;
    r.e = ea * fa + eb * fb;
    r.sx = a.sx * fa + b.sx * fb;
    r.sy = a.sy * fa + b.sy * fb;
    r.srr = a.srr * fa + b.srr * fb;
    return r;
}

// workgroup = 4 waves = 128 queries, wave = 32 queries, key tiles of 64; 2 K slots (tile t+1 lands while tile t is consumed) and
// 2 slots of key coordinates; one workgroup barrier per tile.  Two workgroups per CU (64 KB of LDS each in exact mode).
template <class T, int NS, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void match_stats_kernel(MsArgs a) {
    constexpr int TK = 64;
    constexpr int PLANE = TK * 256;
    constexpr int KSLOT = NS * PLANE;
    constexpr int CSLOT = 2 * TK * 4;            // x[64] | y[64] of a tile's keys
    constexpr int CBASE = 2 * KSLOT;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KSLOT + 2 * CSLOT];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int b = blockIdx.y;
    const int qwg = blockIdx.x * 128;
    const int qi = qwg + wave * 32 + (lane & 31);
    const int qr = min(qi, a.Lq - 1);

    // ---- Q fragments (B operand of S^T = K . Q^T)
    i16x8 qf[NS][8];
    {
        const unsigned short* qb = a.qp + ((long)b * a.Lq + qr) * UM_CHANNELS + 8 * half;
#pragma unroll
        for (int pl = 0; pl < NS; ++pl)
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) qf[pl][ks] = ld_global_16B(qb + pl * a.q_plane_stride + 16 * ks);
    }
    const float qx = (float)(qr % a.gw), qy = (float)(qr / a.gw);

    int ntiles = (a.Lk + TK - 1) / TK;
    if (CAUSAL) ntiles = min(ntiles, (min(qwg + 127, a.Lq - 1) / TK) + 1);

    // ---- staging: wave w moves rows 16w .. 16w+15 of a tile, 4 rows per DMA instruction; rows past the last key repeat it (masked)
    const unsigned kbase_bytes = (unsigned)((long)b * a.Lk * UM_CHANNELS * 2);
    const int srow = 16 * wave + (lane >> 4);
    const int scp = lane & 15;
    auto stage = [&](int t, int slot) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int pl = 0; pl < NS; ++pl) {
                const int row = srow + 4 * j;
                const int key = min(t * TK + row, a.Lk - 1);
                const unsigned off = kbase_bytes + (unsigned)key * (UM_CHANNELS * 2) + ((scp ^ (row & 15)) << 4);
                um_lds_dma16(a.kp + pl * a.k_plane_stride, off, lds + slot * KSLOT + pl * PLANE + (16 * wave + 4 * j) * 256);
            }
        if (wave == 0) {                          // pixel coordinates of the tile's keys
            float* c = reinterpret_cast<float*>(lds + CBASE + slot * CSLOT);
            const int key = t * TK + lane;
            c[lane] = (float)(key % a.gw);
            c[TK + lane] = (float)(key / a.gw);
        }
    };

    int kaddr;
    {
        const int r = lane & 31, x = r & 15;
        kaddr = r * 256 + ((x >> 1) << 5) + ((half ^ (x & 1)) << 4);
    }
    auto frag = [&](const unsigned char* cur, int sub, int pl, int ks) {
        return *reinterpret_cast<const i16x8*>(cur + sub * (32 * 256) + pl * PLANE + (kaddr ^ (ks << 5)));
    };
    // scores of one tile: y0 = keys 0..31, y1 = keys 32..63 (exact mode: lo*hi, hi*lo, hi*hi, as gsv3_kernel orders them)
    auto scores = [&](const unsigned char* cur, f32x16& y0, f32x16& y1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) y0[r] = y1[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                f32x16& y = sub ? y1 : y0;
                const i16x8 hi = frag(cur, sub, 0, ks);
                if (NS == 2) {
                    const i16x8 lo = frag(cur, sub, NS - 1, ks);
                    y = T::mfma(lo, qf[0][ks], y);
                    y = T::mfma(hi, qf[NS - 1][ks], y);
                }
                y = T::mfma(hi, qf[0][ks], y);
            }
    };

    MsState st = ms_empty();
    auto update = [&](f32x16& y0, f32x16& y1, int t, const float* ct) {
        const int kl = t * TK + 4 * half;
        if (CAUSAL || t * TK + TK > a.Lk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kl + (r & 3) + 8 * (r >> 2);
                y0[r] = ((key < a.Lk) && (!CAUSAL || key <= qi)) ? y0[r] : UM_NEG_MASK;
                y1[r] = ((key + 32 < a.Lk) && (!CAUSAL || key + 32 <= qi)) ? y1[r] : UM_NEG_MASK;
            }
        }
        float tm = fmaxf(y0[0], y1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) tm = fmaxf(tm, fmaxf(y0[r], y1[r]));
        // the lowest of this lane's keys that attains the tile maximum (keys ascend with the register index, sub-tile 1 above 0)
        int jt = 0;
#pragma unroll
        for (int r = 15; r >= 0; --r) jt = (y1[r] == tm) ? kl + 32 + (r & 3) + 8 * (r >> 2) : jt;
#pragma unroll
        for (int r = 15; r >= 0; --r) jt = (y0[r] == tm) ? kl + (r & 3) + 8 * (r >> 2) : jt;
        if (tm > st.mt) {                                   // strictly: on a tie the earlier (lower) key stays
            st.e -= (tm - st.mt) * st.l;                    // (empty state: 1e30 * 0)
            st.mt = tm;
            st.j = jt;
            const float Mn = ceilf(tm);
            const float f = fast_exp2(st.M - Mn);           // Mn >= M, both integers: an exact power of two (0 for the empty state)
            st.M = Mn;
            st.l *= f;
            st.e *= f;
            st.sx *= f;
            st.sy *= f;
            st.srr *= f;
        }
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 cx = *reinterpret_cast<const f32x4*>(ct + sub * 32 + 8 * g + 4 * half);
                const f32x4 cy = *reinterpret_cast<const f32x4*>(ct + TK + sub * 32 + 8 * g + 4 * half);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float s = sub ? y1[4 * g + i] : y0[4 * g + i];
                    const float p = fast_exp2(s - st.M);    // masked: 2^-2e30 == 0, and 0 * (finite) below
                    const float dx = cx[i] - qx, dy = cy[i] - qy;
                    st.l += p;
                    st.e = __builtin_fmaf(p, s - st.mt, st.e);
                    st.sx = __builtin_fmaf(p, dx, st.sx);
                    st.sy = __builtin_fmaf(p, dy, st.sy);
                    st.srr = __builtin_fmaf(p, __builtin_fmaf(dx, dx, dy * dy), st.srr);
                }
            }
    };

    if (ntiles > 0) stage(0, 0);
    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile t has landed
        __syncthreads();                                    // ... everyone's; and everyone is done reading the other slot (tile t-1)
        if (t + 1 < ntiles) stage(t + 1, (t + 1) & 1);
        f32x16 y0, y1;
        scores(lds + (t & 1) * KSLOT, y0, y1);
        update(y0, y1, t, reinterpret_cast<const float*>(lds + CBASE + (t & 1) * CSLOT));
    }

    // ---- merge the two half-waves' partial states and write
    MsState o;
    o.M = __shfl_xor(st.M, 32);
    o.mt = __shfl_xor(st.mt, 32);
    o.j = __shfl_xor(st.j, 32);
    o.l = __shfl_xor(st.l, 32);
    o.e = __shfl_xor(st.e, 32);
    o.sx = __shfl_xor(st.sx, 32);
    o.sy = __shfl_xor(st.sy, 32);
    o.srr = __shfl_xor(st.srr, 32);
    const MsState r = ms_merge(st, o);
    if (half != 0 || qi >= a.Lq) return;
    const long plane = (long)a.rows * a.Lq;
    const int img = b / a.rows;
    const long at = (long)(b - img * a.rows) * a.Lq + qi;
    const float pm = fast_exp2(r.mt - r.M);                 // the best key's own term: the same instruction on the same input
    const float mx = r.sx / r.l, my = r.sy / r.l;
    float* so = a.stats + (long)img * 3 * plane + at;
    so[0] = pm / r.l;
    so[plane] = fmaxf(__logf(r.l / pm) - 0.6931471805599453f * (r.e / r.l), 0.f);
    so[2 * plane] = fmaxf(r.srr / r.l - mx * mx - my * my, 0.f);
    a.best[(long)img * plane + at] = r.j;
    if (a.mean) {
        float* mo = a.mean + (long)img * a.nmean * plane + at;
        mo[0] = mx;
        if (a.nmean == 2) mo[plane] = my;
    }
}

// mutual[b, i] = Chebyshev distance between i and best_bwd[b, best_fwd[b, i]] <= radius (0: exact mutual nearest neighbours);
// an index outside [0, L) is no match
__global__ __launch_bounds__(256) void match_mutual_kernel(const int* __restrict__ fwd, const int* __restrict__ bwd,
                                                           unsigned char* __restrict__ out, long total, int L, int w, int radius) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i / L;
    const int q = (int)(i - b * L);
    const int j = fwd[i];
    unsigned char m = 0;
    if (j >= 0 && j < L) {
        const int k = bwd[b * L + j];
        if (k >= 0 && k < L) {
            const int dx = abs(k % w - q % w), dy = abs(k / w - q / w);
            m = max(dx, dy) <= radius ? 1 : 0;
        }
    }
    out[i] = m;
}

// ------------------------------------------------------------------------------------ host side
extern void um_set_error(const char* fmt, ...);

static size_t ms_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// a failed launch: the hipError_t goes back as it is, and um_last_error_string() names the step
static int ms_hip_failed(hipError_t e, const char* what) {
    um_set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

extern "C" size_t um_global_match_stats_workspace_bytes(int batch, int tokens, int channels, int mode) {
    if (batch <= 0 || tokens <= 0 || channels != UM_CHANNELS || (mode != 0 && mode != 1)) return 0;
    return 2 * ms_align256(planes_bytes((long)batch * tokens, mode));
}

template <bool CAUSAL>
static hipError_t launch_match_stats(const MsArgs& a, int nbatch, int mode, hipStream_t stream) {
    dim3 grid((a.Lq + 127) / 128, nbatch), block(256);
    if (mode == 0)
        hipLaunchKernelGGL((match_stats_kernel<Fp16, 2, CAUSAL>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((match_stats_kernel<Bf16, 1, CAUSAL>), grid, block, 0, stream, a);
    return hipGetLastError();
}

extern "C" int um_global_match_stats(const float* f0, const float* f1, float* stats, int* best, float* mean, int batch, int h, int w,
                                     int channels, int bidir, int stereo, int mode, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!f0 || !f1 || !stats || !best || batch <= 0 || h <= 0 || w <= 0) {
        um_set_error("null pointer or non-positive size (batch=%d h=%d w=%d)", batch, h, w);
        return UM_ERR_BAD_ARG;
    }
    if (channels != UM_CHANNELS) {
        um_set_error("channels=%d unsupported (the library is built for %d)", channels, UM_CHANNELS);
        return UM_ERR_BAD_ARG;
    }
    if (mode != 0 && mode != 1) {
        um_set_error("mode=%d is neither UM_MODE_EXACT nor UM_MODE_FAST", mode);
        return UM_ERR_BAD_ARG;
    }
    if (bidir && stereo) {
        um_set_error("bidir=%d with stereo=%d: the backward direction exists for flow only", bidir, stereo);
        return UM_ERR_BAD_ARG;
    }
    const long L = (long)h * w;
    if ((long)batch * L * UM_CHANNELS * 2 >= (1L << 32)) {               // (before any narrowing of L)
        um_set_error("batch*tokens = %ld exceeds the 32-bit plane addressing of this kernel", (long)batch * L);
        return UM_ERR_UNSUPPORTED;
    }
    const size_t need = um_global_match_stats_workspace_bytes(batch, (int)L, channels, mode);
    if (!workspace || workspace_bytes < need) {
        um_set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const long nrows = stereo ? (long)batch * h : batch;                 // the grid's y extent
    if (nrows > 65535) {
        um_set_error("%ld launch rows (batch, or batch*h scanlines for stereo) exceed the grid's 65535", nrows);
        return UM_ERR_UNSUPPORTED;
    }
    unsigned char* ws = (unsigned char*)workspace;
    const size_t pb = ms_align256(planes_bytes(batch * L, mode));
    unsigned short* p0 = (unsigned short*)ws;
    unsigned short* p1 = (unsigned short*)(ws + pb);
    hipError_t e;
    const float pscale = um_global_corr_plane_scale(channels);
    if ((e = launch_split_planes(f0, p0, batch * L, pscale, mode, stream)) != hipSuccess) return ms_hip_failed(e, "um_global_match_stats: operand planes of f0");
    if ((e = launch_split_planes(f1, p1, batch * L, pscale, mode, stream)) != hipSuccess) return ms_hip_failed(e, "um_global_match_stats: operand planes of f1");

    MsArgs a;
    a.qp = p0;
    a.kp = p1;
    a.q_plane_stride = a.k_plane_stride = batch * L * UM_CHANNELS;
    a.stats = stats;
    a.best = best;
    a.mean = mean;
    if (stereo) {                           // every scanline is an independent launch row on a 1-row grid
        a.Lq = a.Lk = w;
        a.gw = w;
        a.rows = h;
        a.nmean = 1;
        if ((e = launch_match_stats<true>(a, batch * h, mode, stream)) != hipSuccess) return ms_hip_failed(e, "um_global_match_stats: match_stats_kernel (stereo)");
        return 0;
    }
    a.Lq = a.Lk = (int)L;
    a.gw = w;
    a.rows = 1;
    a.nmean = 2;
    if ((e = launch_match_stats<false>(a, batch, mode, stream)) != hipSuccess) return ms_hip_failed(e, "um_global_match_stats: match_stats_kernel");
    if (bidir) {                            // f1 -> f0 on the same planes
        a.qp = p1;
        a.kp = p0;
        a.stats = stats + (long)batch * 3 * L;
        a.best = best + (long)batch * L;
        a.mean = mean ? mean + (long)batch * 2 * L : nullptr;
        if ((e = launch_match_stats<false>(a, batch, mode, stream)) != hipSuccess) return ms_hip_failed(e, "um_global_match_stats: match_stats_kernel (backward)");
    }
    return 0;
}

extern "C" int um_match_mutual(const int* best_fwd, const int* best_bwd, unsigned char* mutual, int batch, int h, int w, int radius,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!best_fwd || !best_bwd || !mutual || batch <= 0 || h <= 0 || w <= 0 || radius < 0) {
        um_set_error("um_match_mutual: null pointer, non-positive size or negative radius (batch=%d h=%d w=%d radius=%d)", batch, h, w, radius);
        return UM_ERR_BAD_ARG;
    }
    if ((long)h * w >= (1L << 31)) {
        um_set_error("um_match_mutual: h*w = %ld exceeds the int32 token index", (long)h * w);
        return UM_ERR_UNSUPPORTED;
    }
    const long total = (long)batch * h * w;
    hipLaunchKernelGGL(match_mutual_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, best_fwd, best_bwd, mutual, total,
                       h * w, w, radius);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ms_hip_failed(e, "um_match_mutual: match_mutual_kernel");
}
