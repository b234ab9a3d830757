// Multi-view plane sweep: several source views vote in ONE cost volume before the softmax.   gfx950 / wave64
//
//   um_depth_corr_softmax_multi        S source views, one reference pixel grid, one candidate list -> soft-argmin + statistics
//   um_depth_corr_softmax_multi_rows   the same with the operands named by a row table (further down)
//
// The fusion rule.  Sources s = 0 .. S-1 share the reference pixel p and the inverse-depth candidates c_j; use[s, b] = 0 switches a
// source off for a sample (it is then never read).  For a source that is on,
//   l_sj = the logit of the two-view sweep (K7, local_ops.hip) for (f0_s, f1_s, cam_s): bilinear sample of f1_s with zero padding
//          where candidate j lands, dot with f0_s(p), times 1/sqrt(C) -- the same projection arithmetic in the same order;
//   v_sj = 1 when candidate j has a bilinear corner inside the image of source s (x0 in [-1, w-1] and y0 in [-1, h-1]).
// Fused:  n_j = sum_s v_sj,   l_j = (sum_s v_sj l_sj) / max(1, n_j),   p = softmax_j l_j.
// `out` is the soft-argmin of p (from_argmax: cand[first arg-max]), the four statistics of um_depth_corr_softmax_stats are taken on
// p, best = first arg-max of l, in_view = candidates with n_j >= 1.  The mean runs over the sources that SEE the candidate, so the
// logits stay at the scale the softmax was trained at; it is an unlearned extension (the weights are trained on two views).
// A candidate out of view has l_sj = 0 exactly, so v_sj l_sj = l_sj: the kernels add l_sj and count v_sj.
//   S = 1:        l 1/1 is exact -- bit for bit the result of um_depth_corr_softmax_stats, in the box form and in the gather form (whose
//                 ray and projection K7 associates differently: depth_ray_slots / depth_tap_slots below follow it, and a pixel with a
//                 gathered source reduces in K7's slot order).
//   a source given 2 or 4 times:  2l/2 and 4l/4 are exact -- bit for bit the single-source result.
//   a sample whose sources are all off:  every logit 0, the uniform distribution, in_view 0.
//
// Each source has its own f0_s: after the Transformer's cross-attention the reference frame's tokens depend on the partner view.
// Layouts are source-major (f0, f1 [S, B, h*w, 128], cam [S, B, 30], use [S, B]), so S = 1 is the two-view layout.
//
// Two kernels, the two shapes of K7 with a source loop around the logits and ONE softmax / statistics reduction after it:
//   depth_multi_box_kernel     D <= 64, lane = candidate.  Per source: bounding box of the corners, the dots of f0_s(p) with the box's
//                              f1_s rows once into the wave-private LDS table (DEPTH_BOX rows, reused source after source), every lane
//                              blends its four corners and adds l_sj / v_sj into two registers.  A (pixel, source) whose box exceeds
//                              DEPTH_BOX forms that source's logits by plain gathers (16 slots x 4 quarters) and brings them to
//                              lane = candidate order through the table.  A pixel all of whose sources fitted the box reduces in
//                              lane order (the box body's code); a pixel with a gathered source reduces in slot order (the gather
//                              body's code, the fused logits redistributed through the table) -- the order K7 uses for such a pixel.
//   depth_multi_gather_kernel  D > 64, 16 slots x 4 quarters, LOCAL_MAX_ROUNDS logit and count registers accumulated over sources.
// What does not depend on the source is hoisted out of the loop: the candidates and the lane's 1 / c_j.
#include "common.h"
#include "timing.h"
#include "local_pixel.h"

struct DepthRay { float q0, q1, q2; };

// ray = R (Kinv [x y 1]^T), as K7 forms it
__device__ __forceinline__ DepthRay depth_ray(const float* cm, int x, int y) {
    const float gx = (float)x, gy = (float)y;
    const float r0 = cm[0] * gx + cm[1] * gy + cm[2];
    const float r1 = cm[3] * gx + cm[4] * gy + cm[5];
    const float r2 = cm[6] * gx + cm[7] * gy + cm[8];
    DepthRay q;
    q.q0 = cm[9] * r0 + cm[10] * r1 + cm[11] * r2;
    q.q1 = cm[12] * r0 + cm[13] * r1 + cm[14] * r2;
    q.q2 = cm[15] * r0 + cm[16] * r1 + cm[17] * r2;
    return q;
}

struct DepthTap { float wx, wy; int x0, y0; };

// where the candidate of depth `depth` lands in the source view: K7's projection arithmetic, in its order
__device__ __forceinline__ DepthTap depth_tap(const float* cm, const DepthRay& q, float depth) {
    const float X = q.q0 * depth + cm[18], Y = q.q1 * depth + cm[19], Z = q.q2 * depth + cm[20];
    const float u = cm[21] * X + cm[22] * Y + cm[23] * Z;
    const float v = cm[24] * X + cm[25] * Y + cm[26] * Z;
    const float zz = fmaxf(cm[27] * X + cm[28] * Y + cm[29] * Z, 1e-3f);
    const float sx = fminf(fmaxf(u / zz, -1.0e6f), 1.0e6f);
    const float sy = fminf(fmaxf(v / zz, -1.0e6f), 1.0e6f);
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    DepthTap t;
    t.wx = sx - fx0;
    t.wy = sy - fy0;
    t.x0 = (int)fx0;
    t.y0 = (int)fy0;
    return t;
}

// The same two steps in the association K7's gather form has in the shipped library: there the compiler packs the three rows of the
// ray and of the projection into paired multiplies, so a row is fma(a, b, rn(c * d)) + rn(e * f) where the scalar form above is a
// chain of two fmas.  Written out operation by operation (no contraction), so that one source through the gather form reproduces
// K7's logits bit for bit whatever the compiler makes of the surrounding loop.
// MAINTENANCE: this pins how the compiler rounds K7's gather form today.  K7's source is plain contracted C++, so a compiler upgrade or
// an edit near depth_pixel_gather can change K7's rounding with no logic error on either side; tests/test_depth_multiview_gpu.py::
// test_one_source_is_the_two_view_kernel then fails at D > 64 / oversized boxes, and these two functions are to be re-derived from the
// new K7.  Sharing K7's source instead was tried: splitting depth_pixel_gather changes K7's own code generation.
__device__ __forceinline__ DepthRay depth_ray_slots(const float* cm, int x, int y) {
#pragma clang fp contract(off)
    const float gx = (float)x, gy = (float)y;
    const float r0 = cm[2] + __builtin_fmaf(cm[1], gy, cm[0] * gx);
    const float r1 = cm[5] + __builtin_fmaf(cm[3], gx, cm[4] * gy);
    const float r2 = cm[8] + (cm[6] * gx + cm[7] * gy);
    DepthRay q;
    q.q0 = __builtin_fmaf(r2, cm[11], __builtin_fmaf(r0, cm[9], r1 * cm[10]));
    q.q1 = __builtin_fmaf(r2, cm[14], __builtin_fmaf(r1, cm[13], r0 * cm[12]));
    q.q2 = __builtin_fmaf(r2, cm[17], __builtin_fmaf(r0, cm[15], r1 * cm[16]));
    return q;
}

__device__ __forceinline__ DepthTap depth_tap_slots(const float* cm, const DepthRay& q, float depth) {
#pragma clang fp contract(off)
    const float X = __builtin_fmaf(q.q0, depth, cm[18]), Y = __builtin_fmaf(q.q1, depth, cm[19]), Z = __builtin_fmaf(q.q2, depth, cm[20]);
    const float u = __builtin_fmaf(X, cm[21], Y * cm[22]) + Z * cm[23];
    const float v = __builtin_fmaf(X, cm[24], Y * cm[25]) + Z * cm[26];
    const float zz = fmaxf(__builtin_fmaf(X, cm[27], Y * cm[28]) + Z * cm[29], 1e-3f);
    const float sx = fminf(fmaxf(u / zz, -1.0e6f), 1.0e6f);
    const float sy = fminf(fmaxf(v / zz, -1.0e6f), 1.0e6f);
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    DepthTap t;
    t.wx = sx - fx0;
    t.wy = sy - fy0;
    t.x0 = (int)fx0;
    t.y0 = (int)fy0;
    return t;
}

// l_sj is a rounded product, as in K7: contracted into the accumulation over sources it would make l + l differ from 2 l
__device__ __forceinline__ float depth_logit(float d, float scale) {
#pragma clang fp contract(off)
    return d * scale;
}

__device__ __forceinline__ bool depth_tap_seen(const DepthTap& t, int h, int w) {
    return t.x0 >= -1 && t.x0 < w && t.y0 >= -1 && t.y0 < h;
}

// one candidate by plain gathers: the four bilinear corners fetched from the source's f1 rows (`f1b`: the sample's first row), the
// lane's 32 channels of each; the caller sums the quarters
__device__ __forceinline__ float depth_tap_gather(const f32x4 (&a)[8], const float* __restrict__ f1b, const DepthTap& t, int h, int w,
                                                  int quarter) {
    float d = 0.f;
#pragma unroll
    for (int cy = 0; cy < 2; ++cy)
#pragma unroll
        for (int cx = 0; cx < 2; ++cx) {
            const int yy = t.y0 + cy, xx = t.x0 + cx;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                const float wt = (cx ? t.wx : 1.f - t.wx) * (cy ? t.wy : 1.f - t.wy);
                d += wt * dot32(a, f1b + (long)(yy * w + xx) * UM_CHANNELS + 4 * quarter);
            }
        }
    return d;
}

// Softmax, soft-argmin and statistics of one pixel from logits in slot order (candidate t = 16 r + slot, the 4 quarter lanes of a slot
// hold the same value): the reduction of depth_pixel_gather<true> (local_ops.hip), operation for operation.
template <int ROUNDS>
__device__ __forceinline__ float depth_softmax_slots(float (&logit)[ROUNDS], const float (&cv)[ROUNDS], int rounds, int nd, int slot,
                                                     const float* __restrict__ cand, int from_argmax, int peak_radius,
                                                     DepthPixelStats& st) {
    float mx = -3.0e38f;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (r < rounds) mx = fmaxf(mx, logit[r]);
    mx = slot_max(mx);
    float sp = 0.f, sc = 0.f;
    float sl = 0.f;                                    // sum e (logit - max)
    float best = -3.0e38f;
    int besti = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r < rounds) {
            const int t = r * 16 + slot;
            const float e = t < nd ? __expf(logit[r] - mx) : 0.f;
            sp += e;
            sc += e * cv[r];
            if (t < nd && logit[r] > best) { best = logit[r]; besti = t; }
            sl += t < nd ? e * (logit[r] - mx) : 0.f;
            logit[r] = e;                              // the second pass below needs e, not the logit
        }
    }
    sp = slot_sum(sp);
    sc = slot_sum(sc);
    float res = sc / sp;
    const int mi = slot_min_i((best == mx) ? besti : 0x7fffffff);     // first index attaining the maximum
    const float mu = res;
    float sv = 0.f, sm = 0.f;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r < rounds) {
            const int t = r * 16 + slot;
            const float dc = cv[r] - mu;
            sv += logit[r] * (dc * dc);
            sm += abs(t - mi) <= peak_radius ? logit[r] : 0.f;
        }
    }
    sl = slot_sum(sl);
    sv = slot_sum(sv);
    sm = slot_sum(sm);
    st.max_prob = 1.0f / sp;
    st.entropy = fmaxf(depth_ln(sp) - sl / sp, 0.f);
    st.variance = sv / sp;
    st.peak_mass = sm / sp;
    st.best = mi;
    if (from_argmax) res = cand[mi];
    return res;
}

__device__ __forceinline__ void lds_settle() {         // the wave's LDS accesses so far are done (same wave: LDS executes in order)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------------ D <= 64: lane = candidate
__global__ __launch_bounds__(256) void depth_multi_box_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                              const float* __restrict__ cam, const unsigned char* __restrict__ use,
                                                              const float* __restrict__ cand, float* __restrict__ out,
                                                              float* __restrict__ stats, int* __restrict__ index, int sources,
                                                              int batch, int h, int w, int nd, int from_argmax, int peak_radius) {
    __shared__ float tab_all[4][DEPTH_BOX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane >> 2, quarter = lane & 3;
    float* tab = tab_all[wave];
    const int L = h * w;
    const long total = (long)batch * L;
    const float scale = 1.0f / sqrtf((float)UM_CHANNELS);
    // the lane's candidate does not depend on the pixel or the source
    const bool tap = lane < nd;
    const float ci = cand[tap ? lane : 0];
    const float depth = 1.0f / ci;
    const int rounds = (nd + 15) >> 4;                           // of the gather form: at most 4
    for (long pid = (long)blockIdx.x * 4 + wave; pid < total; pid += (long)gridDim.x * 4) {
        const int b = (int)(pid / L), p = (int)(pid - (long)b * L);
        const int y = p / w, x = p - y * w;
        float acc = 0.f;                                         // sum_s v_sj l_sj of the lane's candidate
        int cnt = 0;                                             // n_j
        bool gathered = false;                                   // wave-uniform: a source of this pixel took the gather form
        for (int s = 0; s < sources; ++s) {
            const long sb = (long)s * batch + b;
            if (use && !use[sb]) continue;                       // wave-uniform; a source that is off is never read
            const float* cm = cam + sb * 30;
            const float* f1b = f1 + sb * L * UM_CHANNELS;
            const DepthRay q = depth_ray(cm, x, y);
            const DepthTap t = depth_tap(cm, q, depth);
            // bounding box of the corners that can lie inside the image: a candidate whose x0 is outside [-1, w-1] has no corner in it
            const int cx0 = min(max(t.x0, -1), w - 1), cy0 = min(max(t.y0, -1), h - 1);
            const int bx0 = wave_min_i(tap ? cx0 : 0x7fffffff), bx1 = wave_max_i(tap ? cx0 + 1 : -0x7fffffff);
            const int by0 = wave_min_i(tap ? cy0 : 0x7fffffff), by1 = wave_max_i(tap ? cy0 + 1 : -0x7fffffff);
            const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
            const int npos = bw * bh;
            f32x4 a[8];
            load32(a, f0 + (sb * L + p) * UM_CHANNELS + 4 * quarter);
            float lg;
            bool seen;                                           // v_sj, from the tap that formed l_sj
            if (npos > DEPTH_BOX) {                              // wave-uniform: this source by plain gathers, 16 candidates per round
                gathered = true;
                for (int r = 0; r < rounds; ++r) {
                    const int tt = r * 16 + slot;
                    const bool on = tt < nd;
                    const DepthTap g = depth_tap_slots(cm, q, 1.0f / cand[on ? tt : 0]);
                    float d = 0.f;
                    if (on) d = depth_tap_gather(a, f1b, g, h, w, quarter);
                    d = quad_sum(d);
                    if (quarter == 0 && on) {                    // tt < nd <= 64 and 64 + tt < 128 <= DEPTH_BOX
                        tab[tt] = depth_logit(d, scale);
                        tab[64 + tt] = depth_tap_seen(g, h, w) ? 1.f : 0.f;     // v_sj of the tap the logit was gathered at, as K7 counts it
                    }
                }
                lds_settle();
                lg = tab[tap ? lane : 0];
                seen = tap && tab[64 + (tap ? lane : 0)] != 0.f;
            } else {
                const float rbw = 1.0f / (float)bw;
                for (int i0 = 0; i0 < npos; i0 += 16) {
                    const int i = i0 + slot;
                    int ry = (int)((float)i * rbw);               // i / bw for 0 <= i < 160, corrected below
                    ry += ((ry + 1) * bw <= i) ? 1 : 0;
                    ry -= (ry * bw > i) ? 1 : 0;
                    const int py = by0 + ry, px = bx0 + (i - ry * bw);
                    float d = 0.f;
                    if (i < npos && py >= 0 && py < h && px >= 0 && px < w)
                        d = dot32(a, f1b + (long)(py * w + px) * UM_CHANNELS + 4 * quarter);
                    d = quad_sum(d);
                    if (quarter == 0 && i < npos) tab[i] = d;
                }
                lds_settle();                                    // the table is complete
                float d = 0.f;
                if (tap) {
#pragma unroll
                    for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                        for (int cx = 0; cx < 2; ++cx) {
                            const int yy = t.y0 + cy, xx = t.x0 + cx;
                            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                                const float wt = (cx ? t.wx : 1.f - t.wx) * (cy ? t.wy : 1.f - t.wy);
                                d += wt * tab[(yy - by0) * bw + (xx - bx0)];
                            }
                        }
                }
                lg = depth_logit(d, scale);
                seen = tap && depth_tap_seen(t, h, w);
            }
            lds_settle();                                        // every lane has read before the next source overwrites the table
            acc += seen ? lg : 0.f;
            cnt += seen ? 1 : 0;
        }
        const float fused = acc / (float)max(cnt, 1);
        const int in_view = __popcll(__ballot(tap && cnt >= 1));
        float res;
        DepthPixelStats st;
        if (gathered) {                                          // the order of K7's gather form: slots x rounds
            if (tap) tab[lane] = fused;
            lds_settle();
            float logit[4], cv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tt = r * 16 + slot;
                const bool on = r < rounds && tt < nd;
                logit[r] = on ? tab[tt] : -3.0e38f;
                cv[r] = r < rounds ? cand[on ? tt : 0] : 0.f;
            }
            lds_settle();
            res = depth_softmax_slots<4>(logit, cv, rounds, nd, slot, cand, from_argmax, peak_radius, st);
        } else {                                                 // the order of K7's box form: one candidate per lane
            const float logit = tap ? fused : -3.0e38f;
            const float mx = wave_max_f(logit);
            const float e = tap ? __expf(logit - mx) : 0.f;
            const float sp = wave_sum_f(e), sc = wave_sum_f(e * ci);
            res = sc / sp;
            const int mi = wave_min_i((tap && logit == mx) ? lane : 0x7fffffff);     // first index attaining the maximum
            const float dc = ci - res;
            const float sl = wave_sum_f(tap ? e * (logit - mx) : 0.f);
            const float sv = wave_sum_f(e * (dc * dc));
            const float sm = wave_sum_f(abs(lane - mi) <= peak_radius ? e : 0.f);
            st.max_prob = 1.0f / sp;
            st.entropy = fmaxf(depth_ln(sp) - sl / sp, 0.f);
            st.variance = sv / sp;
            st.peak_mass = sm / sp;
            st.best = mi;
            if (from_argmax) res = cand[mi];
        }
        st.in_view = in_view;
        if (lane == 0) {
            out[pid] = res;
            depth_stats_store(stats, index, b, p, L, st);
        }
    }
}

// ------------------------------------------------------------------------------------------- D > 64: 16 slots x 4 channel quarters
__global__ __launch_bounds__(256) void depth_multi_gather_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                 const float* __restrict__ cam, const unsigned char* __restrict__ use,
                                                                 const float* __restrict__ cand, float* __restrict__ out,
                                                                 float* __restrict__ stats, int* __restrict__ index, int sources,
                                                                 int batch, int h, int w, int nd, int from_argmax, int peak_radius) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane >> 2, quarter = lane & 3;
    const int L = h * w;
    const long total = (long)batch * L;
    const int rounds = (nd + 15) >> 4;
    const float scale = 1.0f / sqrtf((float)UM_CHANNELS);
    float cv[LOCAL_MAX_ROUNDS], dep[LOCAL_MAX_ROUNDS];           // the slot's candidates and their depths: the same for every pixel
#pragma unroll
    for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
        const int t = r * 16 + slot;
        cv[r] = r < rounds ? cand[t < nd ? t : 0] : 0.f;
        dep[r] = r < rounds ? 1.0f / cv[r] : 0.f;
    }
    for (long pid = (long)blockIdx.x * 4 + wave; pid < total; pid += (long)gridDim.x * 4) {
        const int b = (int)(pid / L), p = (int)(pid - (long)b * L);
        const int y = p / w, x = p - y * w;
        float acc[LOCAL_MAX_ROUNDS];
        int cnt[LOCAL_MAX_ROUNDS];
#pragma unroll
        for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) { acc[r] = 0.f; cnt[r] = 0; }
        for (int s = 0; s < sources; ++s) {
            const long sb = (long)s * batch + b;
            if (use && !use[sb]) continue;                       // wave-uniform; a source that is off is never read
            const float* cm = cam + sb * 30;
            const float* f1b = f1 + sb * L * UM_CHANNELS;
            const DepthRay q = depth_ray_slots(cm, x, y);
            f32x4 a[8];
            load32(a, f0 + (sb * L + p) * UM_CHANNELS + 4 * quarter);
#pragma unroll
            for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
                if (r < rounds) {
                    const bool on = r * 16 + slot < nd;
                    const DepthTap t = depth_tap_slots(cm, q, dep[r]);
                    float d = 0.f;
                    if (on) d = depth_tap_gather(a, f1b, t, h, w, quarter);
                    d = quad_sum(d);
                    const bool seen = on && depth_tap_seen(t, h, w);
                    acc[r] += seen ? depth_logit(d, scale) : 0.f;
                    cnt[r] += seen ? 1 : 0;
                }
            }
        }
        int seen_any = 0;
#pragma unroll
        for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
            if (r < rounds) {
                seen_any += cnt[r] >= 1 ? 1 : 0;
                acc[r] = r * 16 + slot < nd ? acc[r] / (float)max(cnt[r], 1) : -3.0e38f;
            } else {
                acc[r] = -3.0e38f;
            }
        }
        DepthPixelStats st;
        const float res = depth_softmax_slots<LOCAL_MAX_ROUNDS>(acc, cv, rounds, nd, slot, cand, from_argmax, peak_radius, st);
        st.in_view = slot_sum_i(seen_any);
        if (lane == 0) {
            out[pid] = res;
            depth_stats_store(stats, index, b, p, L, st);
        }
    }
}

// ====================================================================================================== operands by row table
//   um_depth_corr_softmax_multi_rows   the same sweep on operands that are ROWS of other tensors (the Transformer's output stream of a
//                                      video chunk), named by a table instead of copied into the source-major layout
// rows [S, B, 3] int32 = f0 row | f1 row | cam row of source s for sample b.  A token row addresses the concatenation of up to
// DEPTH_MAX_SEGMENTS segments [n_i, L, 128]; a cam row addresses cam [cam_rows, 30].  A source any of whose three indices is negative or
// past the end is OFF for the sample and is never read (the `use` of the contiguous entry, and what keeps a bad table in bounds).
// The segment table is a kernel argument, passed by value: first_i is the first row of segment i (INT_MAX for a segment that is not
// there), so the segment of a row is a chain of scalar compares and selects on values read with readfirstlane -- a wave works on one
// pixel, so the three indices are the same in every lane and the base pointers stay in scalar registers.
// The two kernels below are the two kernels above with this addressing, statement for statement: every device function is shared, the
// arithmetic and its order are the same, the results agree bit for bit (tests/test_depth_fuse_neighbours_gpu.py).  They are separate
// kernels and not instantiations of one template because moving the bodies above into templates changed the instructions of
// depth_multi_box_kernel and depth_multi_gather_kernel, whose rounding test_one_source_is_the_two_view_kernel pins.
#define DEPTH_MAX_SEGMENTS 4
struct DepthSegments {                                           // plain members, no arrays: nothing to index, nothing in scratch
    const float *ptr0, *ptr1, *ptr2, *ptr3;
    int first1, first2, first3;
    int total;                                                   // rows of all segments
};

struct DepthSource { const float* cm; const float* f1b; const float* f0b; };     // cam record, first row of the f1 and f0 samples

__device__ __forceinline__ const float* depth_segment_row(const DepthSegments& seg, int r, int L) {      // 0 <= r < seg.total, uniform
    const float* base = seg.ptr0;
    int first = 0;
    if (r >= seg.first1) { base = seg.ptr1; first = seg.first1; }
    if (r >= seg.first2) { base = seg.ptr2; first = seg.first2; }
    if (r >= seg.first3) { base = seg.ptr3; first = seg.first3; }
    return base + (long)(r - first) * L * UM_CHANNELS;
}

__device__ __forceinline__ bool depth_source_rows(const DepthSegments& seg, const float* __restrict__ cam, const int* __restrict__ rows,
                                                  int cam_rows, int s, int b, int batch, int L, DepthSource& o) {
    const int* r = rows + ((long)s * batch + b) * 3;
    const int r0 = __builtin_amdgcn_readfirstlane(r[0]), r1 = __builtin_amdgcn_readfirstlane(r[1]);
    const int rc = __builtin_amdgcn_readfirstlane(r[2]);
    if (r0 < 0 || r1 < 0 || rc < 0 || r0 >= seg.total || r1 >= seg.total || rc >= cam_rows) return false;
    o.cm = cam + (long)rc * 30;
    o.f1b = depth_segment_row(seg, r1, L);
    o.f0b = depth_segment_row(seg, r0, L);
    return true;
}

// ---------------------------------------------------------------------------------------- row table, D <= 64: lane = candidate
__global__ __launch_bounds__(256) void depth_multi_rows_box_kernel(const DepthSegments seg, const float* __restrict__ cam,
                                                                   const int* __restrict__ rows, int cam_rows,
                                                                   const float* __restrict__ cand, float* __restrict__ out,
                                                                   float* __restrict__ stats, int* __restrict__ index, int sources,
                                                                   int batch, int h, int w, int nd, int from_argmax, int peak_radius) {
    __shared__ float tab_all[4][DEPTH_BOX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane >> 2, quarter = lane & 3;
    float* tab = tab_all[wave];
    const int L = h * w;
    const long total = (long)batch * L;
    const float scale = 1.0f / sqrtf((float)UM_CHANNELS);
    // the lane's candidate does not depend on the pixel or the source
    const bool tap = lane < nd;
    const float ci = cand[tap ? lane : 0];
    const float depth = 1.0f / ci;
    const int rounds = (nd + 15) >> 4;                           // of the gather form: at most 4
    for (long pid = (long)blockIdx.x * 4 + wave; pid < total; pid += (long)gridDim.x * 4) {
        const int b = (int)(pid / L), p = (int)(pid - (long)b * L);
        const int y = p / w, x = p - y * w;
        float acc = 0.f;                                         // sum_s v_sj l_sj of the lane's candidate
        int cnt = 0;                                             // n_j
        bool gathered = false;                                   // wave-uniform: a source of this pixel took the gather form
        for (int s = 0; s < sources; ++s) {
            DepthSource src;
            if (!depth_source_rows(seg, cam, rows, cam_rows, s, b, batch, L, src)) continue;     // wave-uniform; off: never read
            const float* cm = src.cm;
            const float* f1b = src.f1b;
            const DepthRay q = depth_ray(cm, x, y);
            const DepthTap t = depth_tap(cm, q, depth);
            // bounding box of the corners that can lie inside the image: a candidate whose x0 is outside [-1, w-1] has no corner in it
            const int cx0 = min(max(t.x0, -1), w - 1), cy0 = min(max(t.y0, -1), h - 1);
            const int bx0 = wave_min_i(tap ? cx0 : 0x7fffffff), bx1 = wave_max_i(tap ? cx0 + 1 : -0x7fffffff);
            const int by0 = wave_min_i(tap ? cy0 : 0x7fffffff), by1 = wave_max_i(tap ? cy0 + 1 : -0x7fffffff);
            const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
            const int npos = bw * bh;
            f32x4 a[8];
            load32(a, src.f0b + (long)p * UM_CHANNELS + 4 * quarter);
            float lg;
            bool seen;                                           // v_sj, from the tap that formed l_sj
            if (npos > DEPTH_BOX) {                              // wave-uniform: this source by plain gathers, 16 candidates per round
                gathered = true;
                for (int r = 0; r < rounds; ++r) {
                    const int tt = r * 16 + slot;
                    const bool on = tt < nd;
                    const DepthTap g = depth_tap_slots(cm, q, 1.0f / cand[on ? tt : 0]);
                    float d = 0.f;
                    if (on) d = depth_tap_gather(a, f1b, g, h, w, quarter);
                    d = quad_sum(d);
                    if (quarter == 0 && on) {                    // tt < nd <= 64 and 64 + tt < 128 <= DEPTH_BOX
                        tab[tt] = depth_logit(d, scale);
                        tab[64 + tt] = depth_tap_seen(g, h, w) ? 1.f : 0.f;     // v_sj of the tap the logit was gathered at, as K7 counts it
                    }
                }
                lds_settle();
                lg = tab[tap ? lane : 0];
                seen = tap && tab[64 + (tap ? lane : 0)] != 0.f;
            } else {
                const float rbw = 1.0f / (float)bw;
                for (int i0 = 0; i0 < npos; i0 += 16) {
                    const int i = i0 + slot;
                    int ry = (int)((float)i * rbw);               // i / bw for 0 <= i < 160, corrected below
                    ry += ((ry + 1) * bw <= i) ? 1 : 0;
                    ry -= (ry * bw > i) ? 1 : 0;
                    const int py = by0 + ry, px = bx0 + (i - ry * bw);
                    float d = 0.f;
                    if (i < npos && py >= 0 && py < h && px >= 0 && px < w)
                        d = dot32(a, f1b + (long)(py * w + px) * UM_CHANNELS + 4 * quarter);
                    d = quad_sum(d);
                    if (quarter == 0 && i < npos) tab[i] = d;
                }
                lds_settle();                                    // the table is complete
                float d = 0.f;
                if (tap) {
#pragma unroll
                    for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                        for (int cx = 0; cx < 2; ++cx) {
                            const int yy = t.y0 + cy, xx = t.x0 + cx;
                            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                                const float wt = (cx ? t.wx : 1.f - t.wx) * (cy ? t.wy : 1.f - t.wy);
                                d += wt * tab[(yy - by0) * bw + (xx - bx0)];
                            }
                        }
                }
                lg = depth_logit(d, scale);
                seen = tap && depth_tap_seen(t, h, w);
            }
            lds_settle();                                        // every lane has read before the next source overwrites the table
            acc += seen ? lg : 0.f;
            cnt += seen ? 1 : 0;
        }
        const float fused = acc / (float)max(cnt, 1);
        const int in_view = __popcll(__ballot(tap && cnt >= 1));
        float res;
        DepthPixelStats st;
        if (gathered) {                                          // the order of K7's gather form: slots x rounds
            if (tap) tab[lane] = fused;
            lds_settle();
            float logit[4], cv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tt = r * 16 + slot;
                const bool on = r < rounds && tt < nd;
                logit[r] = on ? tab[tt] : -3.0e38f;
                cv[r] = r < rounds ? cand[on ? tt : 0] : 0.f;
            }
            lds_settle();
            res = depth_softmax_slots<4>(logit, cv, rounds, nd, slot, cand, from_argmax, peak_radius, st);
        } else {                                                 // the order of K7's box form: one candidate per lane
            const float logit = tap ? fused : -3.0e38f;
            const float mx = wave_max_f(logit);
            const float e = tap ? __expf(logit - mx) : 0.f;
            const float sp = wave_sum_f(e), sc = wave_sum_f(e * ci);
            res = sc / sp;
            const int mi = wave_min_i((tap && logit == mx) ? lane : 0x7fffffff);     // first index attaining the maximum
            const float dc = ci - res;
            const float sl = wave_sum_f(tap ? e * (logit - mx) : 0.f);
            const float sv = wave_sum_f(e * (dc * dc));
            const float sm = wave_sum_f(abs(lane - mi) <= peak_radius ? e : 0.f);
            st.max_prob = 1.0f / sp;
            st.entropy = fmaxf(depth_ln(sp) - sl / sp, 0.f);
            st.variance = sv / sp;
            st.peak_mass = sm / sp;
            st.best = mi;
            if (from_argmax) res = cand[mi];
        }
        st.in_view = in_view;
        if (lane == 0) {
            out[pid] = res;
            depth_stats_store(stats, index, b, p, L, st);
        }
    }
}

// ----------------------------------------------------------------------------- row table, D > 64: 16 slots x 4 channel quarters
__global__ __launch_bounds__(256) void depth_multi_rows_gather_kernel(const DepthSegments seg, const float* __restrict__ cam,
                                                                      const int* __restrict__ rows, int cam_rows,
                                                                      const float* __restrict__ cand, float* __restrict__ out,
                                                                      float* __restrict__ stats, int* __restrict__ index, int sources,
                                                                      int batch, int h, int w, int nd, int from_argmax, int peak_radius) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane >> 2, quarter = lane & 3;
    const int L = h * w;
    const long total = (long)batch * L;
    const int rounds = (nd + 15) >> 4;
    const float scale = 1.0f / sqrtf((float)UM_CHANNELS);
    float cv[LOCAL_MAX_ROUNDS], dep[LOCAL_MAX_ROUNDS];           // the slot's candidates and their depths: the same for every pixel
#pragma unroll
    for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
        const int t = r * 16 + slot;
        cv[r] = r < rounds ? cand[t < nd ? t : 0] : 0.f;
        dep[r] = r < rounds ? 1.0f / cv[r] : 0.f;
    }
    for (long pid = (long)blockIdx.x * 4 + wave; pid < total; pid += (long)gridDim.x * 4) {
        const int b = (int)(pid / L), p = (int)(pid - (long)b * L);
        const int y = p / w, x = p - y * w;
        float acc[LOCAL_MAX_ROUNDS];
        int cnt[LOCAL_MAX_ROUNDS];
#pragma unroll
        for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) { acc[r] = 0.f; cnt[r] = 0; }
        for (int s = 0; s < sources; ++s) {
            DepthSource src;
            if (!depth_source_rows(seg, cam, rows, cam_rows, s, b, batch, L, src)) continue;     // wave-uniform; off: never read
            const float* cm = src.cm;
            const float* f1b = src.f1b;
            const DepthRay q = depth_ray_slots(cm, x, y);
            f32x4 a[8];
            load32(a, src.f0b + (long)p * UM_CHANNELS + 4 * quarter);
#pragma unroll
            for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
                if (r < rounds) {
                    const bool on = r * 16 + slot < nd;
                    const DepthTap t = depth_tap_slots(cm, q, dep[r]);
                    float d = 0.f;
                    if (on) d = depth_tap_gather(a, f1b, t, h, w, quarter);
                    d = quad_sum(d);
                    const bool seen = on && depth_tap_seen(t, h, w);
                    acc[r] += seen ? depth_logit(d, scale) : 0.f;
                    cnt[r] += seen ? 1 : 0;
                }
            }
        }
        int seen_any = 0;
#pragma unroll
        for (int r = 0; r < LOCAL_MAX_ROUNDS; ++r) {
            if (r < rounds) {
                seen_any += cnt[r] >= 1 ? 1 : 0;
                acc[r] = r * 16 + slot < nd ? acc[r] / (float)max(cnt[r], 1) : -3.0e38f;
            } else {
                acc[r] = -3.0e38f;
            }
        }
        DepthPixelStats st;
        const float res = depth_softmax_slots<LOCAL_MAX_ROUNDS>(acc, cv, rounds, nd, slot, cand, from_argmax, peak_radius, st);
        st.in_view = slot_sum_i(seen_any);
        if (lane == 0) {
            out[pid] = res;
            depth_stats_store(stats, index, b, p, L, st);
        }
    }
}

// ------------------------------------------------------------------------------------ host side
extern void um_set_error(const char* fmt, ...);

extern "C" int um_depth_corr_softmax_multi(const float* f0, const float* f1, const float* cam, const unsigned char* use,
                                           const float* candidates, float* out, float* stats, int* index, int sources, int batch,
                                           int h, int w, int channels, int num_candidates, int from_argmax, int peak_radius,
                                           void* stream) {
    if (!f0 || !f1 || !cam || !candidates || !out || batch <= 0 || h <= 0 || w <= 0) {
        um_set_error("um_depth_corr_softmax_multi: null pointer or non-positive size (f0=%p f1=%p cam=%p candidates=%p out=%p batch=%d h=%d w=%d)",
                     (const void*)f0, (const void*)f1, (const void*)cam, (const void*)candidates, (const void*)out, batch, h, w);
        return -1;
    }
    if (channels != UM_CHANNELS) {
        um_set_error("channels=%d unsupported (the library is built for %d)", channels, UM_CHANNELS);
        return -1;
    }
    if (sources < 1 || sources > 8) {
        um_set_error("sources=%d unsupported (1..8)", sources);
        return -4;
    }
    if (num_candidates < 1 || num_candidates > 16 * LOCAL_MAX_ROUNDS) {
        um_set_error("num_candidates=%d unsupported (1..%d)", num_candidates, 16 * LOCAL_MAX_ROUNDS);
        return -4;
    }
    if (peak_radius < 0) {
        um_set_error("peak_radius=%d: the window around the best candidate needs a radius >= 0", peak_radius);
        return -4;
    }
    ScopedKernelTimer timer(UM_K_DEPTH_CORR, (hipStream_t)stream);
    const dim3 grid(pixel_grid_blocks((long)batch * h * w));
    if (num_candidates <= 64)
        hipLaunchKernelGGL(depth_multi_box_kernel, grid, dim3(256), 0, (hipStream_t)stream, f0, f1, cam, use, candidates, out, stats,
                           index, sources, batch, h, w, num_candidates, from_argmax, peak_radius);
    else
        hipLaunchKernelGGL(depth_multi_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, f0, f1, cam, use, candidates, out, stats,
                           index, sources, batch, h, w, num_candidates, from_argmax, peak_radius);
    return (int)hipGetLastError();
}

extern "C" int um_depth_corr_softmax_multi_rows(const float* const* segments, const int* segment_rows, int num_segments,
                                                const float* cam, int cam_rows, const int* rows, const float* candidates, float* out,
                                                float* stats, int* index, int sources, int batch, int h, int w, int channels,
                                                int num_candidates, int from_argmax, int peak_radius, void* stream) {
    if (!segments || !segment_rows || !cam || !rows || !candidates || !out || batch <= 0 || h <= 0 || w <= 0) {
        um_set_error("um_depth_corr_softmax_multi_rows: null pointer or non-positive size (segments=%p segment_rows=%p cam=%p rows=%p candidates=%p out=%p batch=%d h=%d w=%d)",
                     (const void*)segments, (const void*)segment_rows, (const void*)cam, (const void*)rows, (const void*)candidates,
                     (const void*)out, batch, h, w);
        return -1;
    }
    if (num_segments < 1 || num_segments > DEPTH_MAX_SEGMENTS) {
        um_set_error("num_segments=%d unsupported (1..%d)", num_segments, DEPTH_MAX_SEGMENTS);
        return -4;
    }
    if (cam_rows <= 0) {
        um_set_error("cam_rows=%d: the cam table needs at least one row", cam_rows);
        return -4;
    }
    if (channels != UM_CHANNELS) {
        um_set_error("channels=%d unsupported (the library is built for %d)", channels, UM_CHANNELS);
        return -1;
    }
    if (sources < 1 || sources > 8) {
        um_set_error("sources=%d unsupported (1..8)", sources);
        return -4;
    }
    if (num_candidates < 1 || num_candidates > 16 * LOCAL_MAX_ROUNDS) {
        um_set_error("num_candidates=%d unsupported (1..%d)", num_candidates, 16 * LOCAL_MAX_ROUNDS);
        return -4;
    }
    if (peak_radius < 0) {
        um_set_error("peak_radius=%d: the window around the best candidate needs a radius >= 0", peak_radius);
        return -4;
    }
    const float* ptr[DEPTH_MAX_SEGMENTS];
    int first[DEPTH_MAX_SEGMENTS];
    long total_rows = 0;
    for (int i = 0; i < DEPTH_MAX_SEGMENTS; ++i) {
        ptr[i] = nullptr;
        first[i] = 0x7fffffff;                                   // no row index reaches a segment that is not there
        if (i >= num_segments) continue;
        if (!segments[i] || segment_rows[i] <= 0) {
            um_set_error("segment %d: pointer %p with %d rows (every segment needs a pointer and at least one row)", i,
                         (const void*)segments[i], segment_rows[i]);
            return -4;
        }
        ptr[i] = segments[i];
        first[i] = (int)total_rows;
        total_rows += segment_rows[i];
        if (total_rows >= 0x7fffffff) {
            um_set_error("the segments hold %ld rows or more: a row index is a 32-bit int", total_rows);
            return -4;
        }
    }
    DepthSegments seg = {ptr[0], ptr[1], ptr[2], ptr[3], first[1], first[2], first[3], 0};
    seg.total = (int)total_rows;
    ScopedKernelTimer timer(UM_K_DEPTH_CORR, (hipStream_t)stream);
    const dim3 grid(pixel_grid_blocks((long)batch * h * w));
    if (num_candidates <= 64)
        hipLaunchKernelGGL(depth_multi_rows_box_kernel, grid, dim3(256), 0, (hipStream_t)stream, seg, cam, rows, cam_rows, candidates, out,
                           stats, index, sources, batch, h, w, num_candidates, from_argmax, peak_radius);
    else
        hipLaunchKernelGGL(depth_multi_rows_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, seg, cam, rows, cam_rows, candidates,
                           out, stats, index, sources, batch, h, w, num_candidates, from_argmax, peak_radius);
    return (int)hipGetLastError();
}
