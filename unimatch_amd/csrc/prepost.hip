// Inference-size handling around the model: image preparation and prediction restoring.              gfx950 / wave64
//
// The reference's evaluation scripts repeat one block around the forward (evaluate_flow.py:713-758, evaluate_stereo.py:340-375,
// evaluate_depth.py:78-129): transpose tall inputs, pad or resize to the inference size, run the model, crop or resize back, rescale.
//
//   um_image_prepare   images (fp32 NCHW or uint8 NHWC, as a decoder delivers them) -> the model's input [B,3,hp,wp] fp32:
//                      optional transpose, optional (x / 255 - mean) / std, then replicate padding at (top, left) or a bilinear resize.
//   um_pred_restore    prediction [B,C,hp,wp] -> [B,C,h,w]: crop at (top, left) or bilinear resize, the per-kind rescale of the
//                      resize path ((v * ori) / inf), optional transpose back (the flow channels are NOT swapped, as in the reference).
//
//   um_image_prepare_flip / um_pred_restore_flip   the same launches with a mirror of image-space x as the last step (the flipped
//                      views of the reference's stereo inference, evaluate_stereo.py:790-841): an index remap, evaluated with the
//                      mirrored column's arithmetic, so the result is torch.flip of the unflipped one bit for bit.
//
// Both are memory-bound, one launch each, and keep no state.  "Image space" below is the frame after the optional transpose
// (ih x iw): all geometry is expressed there.  Thread mapping:
//   plain       a thread produces VEC (4 or 1) consecutive output pixels of one row and stores them with one 16-byte (4-byte) store
//               per channel; lanes run along the row, so the taps of a wave are one contiguous span of each source row.
//   transposed  the source is contiguous along the OUTPUT's rows.  A workgroup owns a 32 x 32 output tile: in the compute phase its
//               lanes run along the output's y (the source's contiguous direction) and drop the results into an LDS tile, in the store
//               phase they run along x and store 16 bytes each.  No global access is strided.
//
// Bilinear arithmetic is ATen's (UpSampleBilinear2d, align_corners=True) in fp32: scale = float(in - 1) / float(out - 1) (0 for out
// == 1), src = scale * dst, i0 = (int)src, i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1; the two horizontal blends of image
// space first, then the vertical one.  The file is compiled with -ffp-contract=off and IEEE division (build.py): every product, sum and
// quotient is rounded on its own, so the host restatement (unimatch_amd/prepost.py) gives the same bits.
#include "common.h"
#include "timing.h"

extern void um_set_error(const char* fmt, ...);

#define UM_PP_TILE 32

struct PPLerp {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ PPLerp pp_lerp(int dst, float scale, int in) {
    const float src = scale * (float)dst;
    PPLerp r;
    r.i0 = min((int)src, in - 1);              // (src < in for every dst < out: the clamp only guards the address)
    r.i1 = min(r.i0 + 1, in - 1);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

// what both kernels need to place an output pixel in image space
struct PPGeom {
    int ih, iw;            // image-space size of the side that is being sampled
    int mode;              // UM_SIZE_PAD / UM_SIZE_RESIZE
    int top, left;
    float sy, sx;          // resize scales (rows, columns)
};

// ---- um_image_prepare -----------------------------------------------------------------------------------------------------------

struct PrepArgs {
    const void* src;
    float* dst;
    int h, w;              // stored size of a source image
    int hp, wp;
    int tr, norm;
    int flip;              // mirror image-space x: dst[..., x] = prepared[..., wp - 1 - x]
    float mean[3], std[3];
    PPGeom g;
};

// the three channels of image-space pixel (y, x) of image b, normalised when asked
template <int LAYOUT>
__device__ __forceinline__ void prep_fetch(const PrepArgs& a, int b, int y, int x, float v[3]) {
    const int ry = a.tr ? x : y, rx = a.tr ? y : x;
    if (LAYOUT == UM_IMG_U8_NHWC) {
        const unsigned char* p = (const unsigned char*)a.src + (((long)b * a.h + ry) * a.w + rx) * 3;
        v[0] = (float)p[0];
        v[1] = (float)p[1];
        v[2] = (float)p[2];
    } else {
        const long plane = (long)a.h * a.w;
        const float* p = (const float*)a.src + (long)b * 3 * plane + (long)ry * a.w + rx;
        v[0] = p[0];
        v[1] = p[plane];
        v[2] = p[2 * plane];
    }
    if (a.norm) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (v[c] / 255.0f - a.mean[c]) / a.std[c];
    }
}

// (ox is the STORED column: with the mirror the pixel computed is the one of column wp - 1 - ox, with that column's arithmetic)
template <int LAYOUT>
__device__ __forceinline__ void prep_pixel(const PrepArgs& a, int b, int oy, int ox, float out[3]) {
    const PPGeom& g = a.g;
    ox = a.flip ? a.wp - 1 - ox : ox;
    if (g.mode == UM_SIZE_PAD) {
        prep_fetch<LAYOUT>(a, b, min(max(oy - g.top, 0), g.ih - 1), min(max(ox - g.left, 0), g.iw - 1), out);
        return;
    }
    const PPLerp ly = pp_lerp(oy, g.sy, g.ih), lx = pp_lerp(ox, g.sx, g.iw);
    float p00[3], p01[3], p10[3], p11[3];
    prep_fetch<LAYOUT>(a, b, ly.i0, lx.i0, p00);
    prep_fetch<LAYOUT>(a, b, ly.i0, lx.i1, p01);
    prep_fetch<LAYOUT>(a, b, ly.i1, lx.i0, p10);
    prep_fetch<LAYOUT>(a, b, ly.i1, lx.i1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = lx.l0 * p00[c] + lx.l1 * p01[c];
        const float u = lx.l0 * p10[c] + lx.l1 * p11[c];
        out[c] = ly.l0 * t + ly.l1 * u;
    }
}

// plain: block (64, 4), a thread owns VEC pixels of row blockIdx.y * 4 + threadIdx.y
template <int LAYOUT, int VEC>
__global__ __launch_bounds__(256) void image_prepare_kernel(PrepArgs a) {
    const int ox0 = (blockIdx.x * 64 + threadIdx.x) * VEC, oy = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (ox0 >= a.wp || oy >= a.hp) return;
    const long plane = (long)a.hp * a.wp;
    float* o = a.dst + (long)b * 3 * plane + (long)oy * a.wp + ox0;
    if (VEC == 4) {                             // host: wp % 4 == 0 and dst 16-byte aligned
        f32x4 r[3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[3];
            prep_pixel<LAYOUT>(a, b, oy, ox0 + i, v);
            r[0][i] = v[0];
            r[1][i] = v[1];
            r[2][i] = v[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = r[c];
    } else {
        float v[3];
        prep_pixel<LAYOUT>(a, b, oy, ox0, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
    }
}

// store phase of the transposed kernels: tile[C][32][33] holds value (oy - ty0, ox - tx0) at [ox - tx0][oy - ty0]
template <int C>
__device__ __forceinline__ void pp_store_tile(const float (*tile)[UM_PP_TILE][UM_PP_TILE + 1], float* out, long plane, int hout, int wout,
                                              int ty0, int tx0, int vec) {
    const int q = threadIdx.x & 7, r = threadIdx.x >> 3;                       // 8 lanes x 16 bytes cover a tile row, 32 rows
    const int oy = ty0 + r, ox = tx0 + 4 * q;
    if (oy >= hout || ox >= wout) return;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float* o = out + c * plane + (long)oy * wout + ox;
        if (vec && ox + 4 <= wout) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = tile[c][4 * q + i][r];
            *reinterpret_cast<f32x4*>(o) = v;
        } else {
            for (int i = 0; i < 4 && ox + i < wout; ++i) o[i] = tile[c][4 * q + i][r];
        }
    }
}

// transposed: block 256, tile 32 x 32 of the output; compute phase lanes along oy (the source's contiguous direction)
template <int LAYOUT>
__global__ __launch_bounds__(256) void image_prepare_tr_kernel(PrepArgs a, int vec) {
    __shared__ float tile[3][UM_PP_TILE][UM_PP_TILE + 1];
    const int tx0 = blockIdx.x * UM_PP_TILE, ty0 = blockIdx.y * UM_PP_TILE, b = blockIdx.z;
    const int i = threadIdx.x & 31, j0 = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + 8 * k;
        const int oy = ty0 + i, ox = tx0 + j;
        if (oy < a.hp && ox < a.wp) {
            float v[3];
            prep_pixel<LAYOUT>(a, b, oy, ox, v);
            tile[0][j][i] = v[0];
            tile[1][j][i] = v[1];
            tile[2][j][i] = v[2];
        }
    }
    __syncthreads();
    const long plane = (long)a.hp * a.wp;
    pp_store_tile<3>(tile, a.dst + (long)b * 3 * plane, plane, a.hp, a.wp, ty0, tx0, vec);
}

static inline float pp_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

// rows of either side go to grid.y in groups of four (plain) or 32 (transposed), the planes to grid.z: both end at 65535
static inline bool pp_size_ok(int batch, int channels, int h, int w, int hp, int wp) {
    return batch > 0 && channels > 0 && (long)batch * channels <= 65535 && h > 0 && w > 0 && hp > 0 && wp > 0 &&
           h <= UM_PREPOST_MAX_DIM && w <= UM_PREPOST_MAX_DIM && hp <= UM_PREPOST_MAX_DIM && wp <= UM_PREPOST_MAX_DIM &&
           (long)h * w <= (1L << 28) && (long)hp * wp <= (1L << 28);
}

extern "C" int um_image_prepare_flip(const void* src, int src_layout, float* dst, int batch, int h, int w, int transpose,
                                     const float* mean, const float* std, int mode, int hp, int wp, int top, int left, int hflip,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    bool ok = src && dst && pp_size_ok(batch, 3, h, w, hp, wp) && (src_layout == UM_IMG_F32_NCHW || src_layout == UM_IMG_U8_NHWC) &&
              (mode == UM_SIZE_PAD || mode == UM_SIZE_RESIZE) && ((mean == nullptr) == (std == nullptr));
    const int ih = transpose ? w : h, iw = transpose ? h : w;
    if (ok && mode == UM_SIZE_PAD) ok = top >= 0 && left >= 0 && (long)top + ih <= hp && (long)left + iw <= wp;
    if (ok && std)
        for (int c = 0; c < 3; ++c) ok = ok && std[c] != 0.0f && std[c] == std[c] && mean[c] == mean[c];
    if (!ok) {
        um_set_error("um_image_prepare: bad argument (layout=%d batch=%d h=%d w=%d mode=%d hp=%d wp=%d top=%d left=%d)", src_layout,
                     batch, h, w, mode, hp, wp, top, left);
        return UM_ERR_BAD_ARG;
    }
    PrepArgs a;
    a.src = src;
    a.dst = dst;
    a.h = h;
    a.w = w;
    a.hp = hp;
    a.wp = wp;
    a.tr = transpose ? 1 : 0;
    a.norm = mean ? 1 : 0;
    a.flip = hflip ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean ? mean[c] : 0.0f;
        a.std[c] = std ? std[c] : 1.0f;
    }
    a.g = PPGeom{ih, iw, mode, top, left, pp_scale(ih, hp), pp_scale(iw, wp)};
    const int vec = (wp % 4 == 0) && ((uintptr_t)dst % 16 == 0);
    const bool u8 = src_layout == UM_IMG_U8_NHWC;
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    if (a.tr) {
        const dim3 grid((unsigned)((wp + UM_PP_TILE - 1) / UM_PP_TILE), (unsigned)((hp + UM_PP_TILE - 1) / UM_PP_TILE), (unsigned)batch);
        if (u8)
            hipLaunchKernelGGL(image_prepare_tr_kernel<UM_IMG_U8_NHWC>, grid, dim3(256), 0, stream, a, vec);
        else
            hipLaunchKernelGGL(image_prepare_tr_kernel<UM_IMG_F32_NCHW>, grid, dim3(256), 0, stream, a, vec);
    } else {
        const int per = vec ? 256 : 64;
        const dim3 grid((unsigned)((wp + per - 1) / per), (unsigned)((hp + 3) / 4), (unsigned)batch), block(64, 4);
        if (u8 && vec)
            hipLaunchKernelGGL((image_prepare_kernel<UM_IMG_U8_NHWC, 4>), grid, block, 0, stream, a);
        else if (u8)
            hipLaunchKernelGGL((image_prepare_kernel<UM_IMG_U8_NHWC, 1>), grid, block, 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((image_prepare_kernel<UM_IMG_F32_NCHW, 4>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((image_prepare_kernel<UM_IMG_F32_NCHW, 1>), grid, block, 0, stream, a);
    }
    return (int)hipGetLastError();
}

// ---- um_pred_restore ------------------------------------------------------------------------------------------------------------

struct RestArgs {
    const float* pred;
    float* out;
    int channels, hp, wp;
    int h, w;              // stored size of an output plane
    int scaled;            // resize path of a flow / disparity: (v * mul[c]) / div[c]
    int flip;              // mirror the stored x: out[..., x] = restored[..., w - 1 - x]
    float mul[2], div[2];
    PPGeom g;              // ih, iw: the PREDICTION's size (hp, wp); the output in image space is rh x rw
};

// image-space output pixel (y, x) of plane z = b * channels + c
__device__ __forceinline__ float rest_pixel(const RestArgs& a, int z, int c, int y, int x) {
    const float* p = a.pred + (long)z * a.hp * a.wp;
    const PPGeom& g = a.g;
    if (g.mode == UM_SIZE_PAD) return p[(long)(y + g.top) * a.wp + x + g.left];
    const PPLerp ly = pp_lerp(y, g.sy, a.hp), lx = pp_lerp(x, g.sx, a.wp);
    const float* r0 = p + (long)ly.i0 * a.wp;
    const float* r1 = p + (long)ly.i1 * a.wp;
    const float t = lx.l0 * r0[lx.i0] + lx.l1 * r0[lx.i1];
    const float u = lx.l0 * r1[lx.i0] + lx.l1 * r1[lx.i1];
    float v = ly.l0 * t + ly.l1 * u;
    if (a.scaled) v = (v * a.mul[c]) / a.div[c];
    return v;
}

template <int VEC>
__global__ __launch_bounds__(256) void pred_restore_kernel(RestArgs a) {
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * VEC, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (x0 >= a.w || y >= a.h) return;
    const int c = z % a.channels;
    float* o = a.out + ((long)z * a.h + y) * a.w + x0;
    if (VEC == 4) {                             // host: w % 4 == 0 and out 16-byte aligned
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = rest_pixel(a, z, c, y, a.flip ? a.w - 1 - (x0 + i) : x0 + i);
        *reinterpret_cast<f32x4*>(o) = r;
    } else {
        o[0] = rest_pixel(a, z, c, y, a.flip ? a.w - 1 - x0 : x0);
    }
}

// transposed: out[oy][ox] is image-space pixel (ox, oy); lanes of the compute phase run along oy = the prediction's columns
__global__ __launch_bounds__(256) void pred_restore_tr_kernel(RestArgs a, int vec) {
    __shared__ float tile[1][UM_PP_TILE][UM_PP_TILE + 1];
    const int tx0 = blockIdx.x * UM_PP_TILE, ty0 = blockIdx.y * UM_PP_TILE, z = blockIdx.z;
    const int c = z % a.channels;
    const int i = threadIdx.x & 31, j0 = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + 8 * k;
        const int oy = ty0 + i, ox = tx0 + j;
        if (oy < a.h && ox < a.w) tile[0][j][i] = rest_pixel(a, z, c, a.flip ? a.w - 1 - ox : ox, oy);
    }
    __syncthreads();
    const long plane = (long)a.h * a.w;
    pp_store_tile<1>(tile, a.out + (long)z * plane, plane, a.h, a.w, ty0, tx0, vec);
}

extern "C" int um_image_prepare(const void* src, int src_layout, float* dst, int batch, int h, int w, int transpose, const float* mean,
                                const float* std, int mode, int hp, int wp, int top, int left, void* stream) {
    return um_image_prepare_flip(src, src_layout, dst, batch, h, w, transpose, mean, std, mode, hp, wp, top, left, 0, stream);
}

extern "C" int um_pred_restore_flip(const float* pred, float* out, int batch, int channels, int hp, int wp, int mode, int top, int left,
                                    int h, int w, int kind, int transpose, int hflip, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    bool ok = pred && out && pp_size_ok(batch, channels, h, w, hp, wp) && (mode == UM_SIZE_PAD || mode == UM_SIZE_RESIZE) &&
              ((kind == UM_PRED_FLOW && channels == 2) || ((kind == UM_PRED_DISPARITY || kind == UM_PRED_DEPTH) && channels == 1));
    const int rh = transpose ? w : h, rw = transpose ? h : w;          // the restored size in image space
    if (ok && mode == UM_SIZE_PAD) ok = top >= 0 && left >= 0 && (long)top + rh <= hp && (long)left + rw <= wp;
    if (!ok) {
        um_set_error("um_pred_restore: bad argument (batch=%d channels=%d hp=%d wp=%d mode=%d top=%d left=%d h=%d w=%d kind=%d)", batch,
                     channels, hp, wp, mode, top, left, h, w, kind);
        return UM_ERR_BAD_ARG;
    }
    RestArgs a;
    a.pred = pred;
    a.out = out;
    a.channels = channels;
    a.hp = hp;
    a.wp = wp;
    a.h = h;
    a.w = w;
    a.scaled = (mode == UM_SIZE_RESIZE && kind != UM_PRED_DEPTH) ? 1 : 0;
    a.flip = hflip ? 1 : 0;
    a.mul[0] = (float)rw;                       // flow u and disparity: * W / wp;  flow v: * H / hp
    a.div[0] = (float)wp;
    a.mul[1] = (float)rh;
    a.div[1] = (float)hp;
    a.g = PPGeom{hp, wp, mode, top, left, pp_scale(hp, rh), pp_scale(wp, rw)};
    const int vec = (w % 4 == 0) && ((uintptr_t)out % 16 == 0);
    const unsigned planes = (unsigned)(batch * channels);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    if (transpose) {
        const dim3 grid((unsigned)((w + UM_PP_TILE - 1) / UM_PP_TILE), (unsigned)((h + UM_PP_TILE - 1) / UM_PP_TILE), planes);
        hipLaunchKernelGGL(pred_restore_tr_kernel, grid, dim3(256), 0, stream, a, vec);
    } else {
        const int per = vec ? 256 : 64;
        const dim3 grid((unsigned)((w + per - 1) / per), (unsigned)((h + 3) / 4), planes), block(64, 4);
        if (vec)
            hipLaunchKernelGGL(pred_restore_kernel<4>, grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL(pred_restore_kernel<1>, grid, block, 0, stream, a);
    }
    return (int)hipGetLastError();
}

extern "C" int um_pred_restore(const float* pred, float* out, int batch, int channels, int hp, int wp, int mode, int top, int left, int h,
                               int w, int kind, int transpose, void* stream) {
    return um_pred_restore_flip(pred, out, batch, channels, hp, wp, mode, top, left, h, w, kind, transpose, 0, stream);
}
