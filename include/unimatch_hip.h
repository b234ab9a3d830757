/*
 * unimatch_hip.h — C ABI of the MI355X (gfx950) global-matching hot path.
 *
 * The reference (autonomousvision/unimatch) has no FFI: its hot path is a set of Python functions
 * made of ATen ops.  Each entry point below replaces ONE of those functions with one fused HIP
 * launch sequence; the citation on each is the reference function it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - Plain C: pointers and sizes only, no torch types.  All pointers are DEVICE pointers.
 *   - The caller owns every buffer (inputs, outputs, workspace).  The library never allocates or
 *     frees device memory and never keeps a pointer after the call returns.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and performs no host synchronisation.  Stateless and re-entrant.
 *   - Return value: 0 = enqueued; negative = argument error (UM_ERR_*); positive = hipError_t.
 *     um_last_error_string() describes the last failure on the calling thread.
 *   - Feature tensors are "token major": [N, L, C] fp32, L = h*w tokens in row-major (y, x) order,
 *     C = 128 channels contiguous per token (the transpose of the reference's [N, C, h, w]).
 *     Flow-like outputs are [N, V, h, w] fp32 exactly as the reference returns them.
 *   - `mode` selects the operand precision of the MFMA contractions:
 *       UM_MODE_EXACT  fp16 hi+lo split operands, 3 MFMA products per tile, fp32 accumulate
 *                      (~2^-22 relative operand error: meets the fp32 reference to its own noise floor)
 *       UM_MODE_FAST   bf16 operands, 1 MFMA product per tile, fp32 accumulate
 *     Softmax, accumulators and all non-MFMA kernels are fp32 in both modes.
 *   - Operand range (UM_MODE_EXACT): x = hi + lo with hi = rn_fp16(x), lo = rn_fp16(x - hi) gives 22 significant bits
 *     while lo stays in fp16's normal range, i.e. for element magnitudes in about [2^-3, 2^15]; below, the absolute
 *     error floor is 2^-25 (fp16 subnormal granularity), above 65504 the hi plane saturates to inf.  Weights are
 *     pre-scaled by 2^wshift (2^10) so that |w| in [2^-13, 2^5) is covered.  The model's activations on this path are
 *     O(1)..O(10) (LayerNorm / InstanceNorm outputs, features of std 1..4); tests/test_hip_parity_gpu.py sweeps
 *     0.1 .. 100.  There is no per-tensor rescaling: callers with other magnitudes scale by a power of two around the call.
 *     An element of magnitude >= 65504 on its way into an fp16 operand is NOT silent (round 5): the kernel that converts it raises
 *     a bit of a sticky, process-wide flag word (um_range_flags below) that says which kind of operand it was.
 */
#ifndef UNIMATCH_HIP_H
#define UNIMATCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UM_VERSION 220   /* 220 also gained um_global_match_stats_workspace_bytes, um_global_match_stats and um_match_mutual,
                            um_depth_corr_softmax_multi, um_depth_corr_softmax_multi_rows, and the TSDF fusion entry points
                            um_tsdf_integrate, um_tsdf_points_workspace_bytes, um_tsdf_points, um_tsdf_mesh_workspace_bytes and
                            um_tsdf_mesh (additions only: no existing entry point changed, so the number stays) */

#define UM_MODE_EXACT 0
#define UM_MODE_FAST 1

#define UM_ERR_BAD_ARG (-1)      /* null pointer, non-positive size, unsupported channel count ... */
#define UM_ERR_BAD_GEOMETRY (-2) /* window does not tile the map, shift >= window ...             */
#define UM_ERR_WORKSPACE (-3)    /* workspace missing or too small                                  */
#define UM_ERR_UNSUPPORTED (-4)  /* valid in the reference but not implemented by this library      */
#define UM_ERR_COLLECTIVE (-5)   /* RCCL reported an error / the communicator bootstrap failed       */

int um_version(void);
const char* um_last_error_string(void);

/* Operand-range flags (UM_MODE_EXACT only; bf16 operands have fp32's exponent range).  Kernels on the Transformer / matching path
 * that turn fp32 values into fp16 hi | lo operands track the largest magnitude they convert and OR a bit into one sticky word in
 * pinned host memory when it reaches 65504 (the hi plane would be inf and NaN follows downstream; the fp32 reference has no such
 * limit -- unimatch/transformer.py:58-60).  Reading the word costs no device synchronisation; it reflects every launch that has
 * FINISHED, so read it after synchronising the stream(s) when the answer must cover the last call.  `reset` != 0 clears it.
 * The convolution kernels of the CNN encoder / refinement block are not instrumented (instance-normalised / bounded inputs). */
#define UM_RANGE_PLANES 1u        /* um_*_fwd entry points that split whole fp32 tensors (q, k, v, features): split_planes_kernel */
#define UM_RANGE_ATTN_TOKENS 2u   /* um_window_attn_qproj_merge_fwd: the source tokens x                                       */
#define UM_RANGE_ATTN_QUERY 4u    /* ... its projected queries Wq.x                                                           */
#define UM_RANGE_ATTN_OUTPUT 8u   /* um_window_attn_*merge*_fwd: the attention output fed to the merge Linear                 */
#define UM_RANGE_FFN_TOKENS 16u   /* um_ffn_*fwd: the concatenated input [x | y]                                              */
#define UM_RANGE_FFN_HIDDEN 32u   /* ... the hidden activations gelu(W1.[x | y])                                              */
#define UM_RANGE_KV_TOKENS 64u    /* um_kv4_fwd / the k | v epilogue of um_ffn_kv_fwd: tokens, and the projected keys / values;
                                     the token planes of um_ffn_planes_fwd                                                   */
#define UM_RANGE_LINEAR 128u      /* um_linear_fwd: fp32 inputs and plane outputs                                             */
int um_range_flags(unsigned* flags_out, int reset);

/* =============================================================================================
 * MEASUREMENT ABI (um_timing_*, um_census_*): not part of the reference's operator interface.  It exists so that bench.py and
 * the parity tests can (a) time individual kernels with hipEvents on the stream they are launched on and (b) assert which
 * kernel instantiation served a call.  Both are OFF by default; while off the library keeps no state at all and every
 * entry point below is a pure function of its arguments.  Micro-benchmarks of the hardware itself (um_debug_*) are NOT in
 * the shipped library: they live in diagnostic builds only (end of this header).
 * =============================================================================================
 * Kernel timing: when enabled, every launch of the kernels below is bracketed by a pair of
 * hipEvents recorded on the launch stream itself; um_timing_collect() waits for them, returns the summed
 * kernel time and launch count since the last collect, and recycles the events.  Off by default (then the
 * library keeps no state at all).  Two event records per launch are not free (~6 % of a 14 ms forward with every
 * kernel timed): select only the kernels of interest inside a timed region. */
#define UM_K_WINDOW_ATTN 0   /* window_attn_kernel (um_window_attn_fwd)                                  */
#define UM_K_GLOBAL_SOFTMAX 1 /* gsv_kernel (um_global_corr_softmax_flow/_stereo, um_prop_global_attn)    */
#define UM_K_SPLIT_PLANES 2  /* split_planes_kernel (operand conversion pre-pass of the MFMA kernels)     */
#define UM_K_LOCAL_CORR 3    /* local_corr_softmax_kernel                                                */
#define UM_K_COST_VOLUME 4   /* local_corr_with_flow_kernel                                              */
#define UM_K_PROP_LOCAL 5    /* prop_local_attn_kernel                                                   */
#define UM_K_DEPTH_CORR 6    /* depth_corr_softmax_kernel                                                */
#define UM_K_LINEAR 7        /* linear_kernel (um_linear_fwd)                                            */
#define UM_K_INSTANCE_NORM 8 /* instance_norm_kernel (um_instance_norm_fwd)                              */
#define UM_K_CONVEX_UPSAMPLE 9 /* convex_upsample_kernel (um_convex_upsample)                            */
#define UM_K_FFN 10          /* ffn_kernel (um_ffn_fwd)                                                  */
#define UM_K_CONV 11         /* conv_kernel (um_conv2d_fwd)                                              */
#define UM_K_COUNT 12
/* Launch census (diagnostic, off by default): with um_census_enable(1) every launch below counts the kernel INSTANTIATION that
 * served it, so a test can assert that the configuration it checks ran the same kernels the bench times (and not, say, the
 * small-launch split variants).  um_census_enable(1) also zeroes the counters; um_census_count(v) reads one. */
#define UM_V_WATTN_TILE 0     /* window_attn_kernel, one workgroup per 128-query tile                                   */
#define UM_V_WATTN_KSPLIT 1   /* window_attn_kernel<..., KSPLIT>: 2 / 4 workgroups share a query tile (small launches)  */
#define UM_V_FFN_TILE 2       /* ffn_kernel, one workgroup per 128-token tile                                           */
#define UM_V_FFN_HSPLIT 3     /* ffn_kernel<..., HSPLIT>: hidden slices split over 2 / 4 workgroups (small launches)    */
#define UM_V_GSV4 4           /* gsv4_kernel (stream-K global correlation / propagation)                                */
#define UM_V_GSV3 5           /* gsv3_kernel (causal / ragged / small launches)                                         */
#define UM_V_K4_MFMA 6        /* k4m_kernel cost volume (matrix cores, per-tile gather path inside)                      */
#define UM_V_K4_VALU 7        /* local_corr_with_flow_kernel cost volume (VALU)                                         */
#define UM_V_K3_MFMA 8        /* local correlation softmax on k4m_kernel                                                */
#define UM_V_K3_VALU 9        /* local_corr_softmax_kernel (VALU)                                                       */
#define UM_V_CONV_PATCH 10    /* conv_patch_kernel (3x3 stride 1, 2-D halo patch)                                       */
#define UM_V_CONV_ROWS 11     /* conv_rows_kernel (row window shared by the horizontal taps)                            */
#define UM_V_CONV_GENERIC 12  /* conv_kernel (tap-by-tap implicit GEMM)                                                 */
#define UM_V_WATTN_W8 13      /* reserved: an 8-wave attention variant measured and dropped in round 5 (never counted) */
#define UM_V_CONV_PATCH_NORM 14 /* conv_patch_norm_kernel: the patch kernel normalising on load (ALSO counted as UM_V_CONV_PATCH) */
#define UM_V_COUNT 15
int um_census_enable(int on);
long um_census_count(int variant);
/* Key-tile census of the window attention (round 6; diagnostic, off by default).  In a window that carries the shifted-window mask
 * (unimatch/utils.py:84-108) a (128-query workgroup, 32-key tile) pair whose classes differ holds nothing but -100 logits
 * (unimatch/attention.py:88-89); the kernel walks such windows class by class, PROBES those tiles (hi.hi product only) after the
 * workgroup's own-class tiles and drops a tile iff every probed logit stays UM margin (40 natural-log units) below the running
 * row maximum -- otherwise the tile is computed exactly as an unmasked one.  While enabled, every workgroup adds to four counters
 * of the current device: [0] key tiles computed in full, [1] tiles probed, [2] probed tiles that then had to be computed (they are
 * part of [0] as well), [3] workgroups.  um_window_attn_tile_census(enable, counts4): counts4 != NULL synchronises the device,
 * copies the counters out and zeroes them; then the census is switched on / off as `enable` says. */
int um_window_attn_tile_census(int enable, unsigned long long* counts4);
/* Box probes (round 6, csrc/probe.hip): three kernels bench.py times inside its own run so that a bench line describes the box it was
 * measured on (MI355X boxes of one pool differ by several per cent in what they sustain).  Asynchronous on `stream`; the caller times them.
 *   um_probe_mfma(sink, iters): a memory-free loop of independent 32x32x16 fp16 MFMAs with pseudo-random operands on every SIMD;
 *                               executes um_probe_mfma_flops(iters) FLOPs.  sink: one float of device memory (never written).
 *   um_probe_copy(src, dst, bytes): float4 copy, bytes a multiple of 16 (reads `bytes`, writes `bytes`).
 *   um_probe_chase(ring, out, hops): one lane follows ring[i] -> next index for `hops` dependent loads (the caller builds the ring). */
double um_probe_mfma_flops(int iters);
int um_probe_mfma(float* sink, int iters, void* stream);
int um_probe_copy(const void* src, void* dst, size_t bytes, void* stream);
int um_probe_chase(const unsigned* ring, unsigned* out, int hops, void* stream);
int um_timing_enable(int kernel_mask);   /* bit k set: time kernel id UM_K_* = k; -1: all; 0: off */
int um_timing_collect(int kernel_id, double* total_ms, int* launches);
/* ===================================== end of the measurement ABI ============================= */

/* ---------------------------------------------------------------------------------------------
 * Windowed single-head attention  softmax(q k^T / sqrt(C) + shift_mask) v   inside windows.
 * Replaces (one geometry each):
 *   unimatch/attention.py:45-104  single_head_split_window_attention   win=(h/K,w/K), shift=win/2|0
 *   unimatch/attention.py:8-16    single_head_full_attention           win=(h,w)
 *   unimatch/attention.py:19-42   single_head_full_attention_1d        win=(1,w)
 *   unimatch/attention.py:107-163 single_head_split_window_attention_1d win=(1,w/K), shift=(0,win_w/2)|0
 * together with torch.roll, split_feature/merge_splits (unimatch/utils.py:34-81,155-196) and the
 * additive -100 masks (unimatch/utils.py:84-108,199-216), which become index arithmetic.
 * q, k, v, out: [streams, h*w, C] fp32.  C must be 128.
 * ------------------------------------------------------------------------------------------- */
size_t um_window_attn_workspace_bytes(int streams, int tokens, int channels, int mode);
int um_window_attn_fwd(const float* q, const float* k, const float* v, float* out,
                       int streams, int h, int w, int channels,
                       int win_h, int win_w, int shift_h, int shift_w,
                       int mode, void* workspace, size_t workspace_bytes, void* stream);

/* Same attention core on operands that are ALREADY in the MFMA plane format ([NS][rows][ld] 16-bit, NS = 2 fp16
 * planes hi|lo in UM_MODE_EXACT, 1 bf16 plane in UM_MODE_FAST; plane stride = rows * ld elements), e.g. the output
 * of um_linear_fwd(epilogue = UM_EPI_PLANES).  q/k/v may be column slices of wider projections: ldq / ldkv are
 * the row strides in elements (multiples of 8), rows = streams * h * w.  k and v share ldkv.  No workspace.
 * kv_rotate: stream s reads the keys / values of stream (s + kv_rotate) mod streams -- with streams = 2B and kv_rotate = B this
 * is the reference's cross attention of [f0; f1] against [f1; f0] (unimatch/transformer.py:271-291) without the swapped copy. */
int um_window_attn_planes_fwd(const void* q_planes, const void* k_planes, const void* v_planes, float* out,
                              int streams, int h, int w, int channels, int ldq, int ldkv,
                              long q_plane_stride, long kv_plane_stride,
                              int win_h, int win_w, int shift_h, int shift_w, int kv_rotate, int mode, void* stream);

/* um_window_attn_planes_fwd with the layer's tail folded into the epilogue (unimatch/transformer.py:137-138, 144):
 *     out = LayerNorm(attention . Wm^T; gamma, beta, eps) (+ residual)
 * wm_planes: um_weight_planes() of the merge weight [128,128] with `wshift`; residual: optional fp32 [streams*h*w][128]
 * (the self-attention layers' `source + message`).  The attention output never reaches HBM. */
int um_window_attn_merge_fwd(const void* q_planes, const void* k_planes, const void* v_planes, const void* wm_planes,
                             const float* gamma, const float* beta, const float* residual, float eps, int wshift, float* out,
                             int streams, int h, int w, int channels, int ldq, int ldkv, long q_plane_stride,
                             long kv_plane_stride, int win_h, int win_w, int shift_h, int shift_w, int kv_rotate, int mode,
                             void* stream);

/* Same, with the query projection of unimatch/transformer.py:58 folded into the kernel's prologue:
 *     q = x . Wq^T   for the workgroup's 128 query tokens, straight into the MFMA operand registers
 * x: fp32 [streams*h*w][128] source tokens; wq_planes: um_weight_planes() of the query weight [128,128] with the same
 * `wshift` as wm_planes.  A query row is consumed by exactly one workgroup, so nothing is recomputed and the q operand
 * planes (one write + one read of [streams*h*w][128] per layer) never exist; k / v planes as above.
 * workspace (optional, NULL = none): um_window_attn_ksplit_workspace_bytes() bytes that are ZERO before the first launch
 * (the kernel leaves them zero; one workspace serves one launch at a time, launches on one stream are fine).  With it, a
 * launch of few query tiles (batch 1: 40 - 96 workgroups on 256 CUs, each walking a whole window) gives every query tile
 * to 2 or 4 neighbouring workgroups, each on its share of the window's keys; the first merges the others' partial softmaxes
 * (exact).  The byte count is 0 for launches that are not split. */
/* Split launches.  um_window_attn_qproj_merge_fwd and um_ffn_ws_fwd with `workspace` let several workgroups share the key walk of a
 * query tile / the hidden slices of a token tile when the launch is small (launch plans: um_window_attn_plan,
 * um_ffn_split_workspace_bytes).  Every part publishes its partial result in the workspace and takes a ticket from the tile's arrival
 * counter; the last arriver combines all parts in part order (exact / fixed order: bitwise reproducible) and finishes the layer.
 * Nobody waits for anybody: no assumption about residency or dispatch order.  The workspace must be zero before the first launch
 * that uses it, is left with zero counters by every launch, and must not be shared by launches in flight on different streams. */
size_t um_window_attn_ksplit_workspace_bytes(int streams, int h, int w, int win_h, int win_w);
/* The launch plan of um_window_attn_qproj_merge_fwd for a geometry, a pure function of the arguments and the current device's CU
 * count: `full_tiles` 128-query tiles are served one workgroup each, `split_tiles` tiles by `parts` workgroups each on a share of
 * the window's key tiles (launches whose tiles all fit the chip at once: batch-1 latency; big launches are never split -- measured). */
int um_window_attn_plan(int streams, int h, int w, int win_h, int win_w, int* full_tiles, int* split_tiles, int* parts);
int um_window_attn_qproj_merge_fwd(const float* x, const void* wq_planes, const void* k_planes, const void* v_planes,
                                   const void* wm_planes, const float* gamma, const float* beta, const float* residual, float eps,
                                   int wshift, float* out, int streams, int h, int w, int channels, int ldkv,
                                   long kv_plane_stride, int win_h, int win_w, int shift_h, int shift_w, int kv_rotate, int mode,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Transformer-layer linears  C[M,N] = A[M,K] . W[N,K]^T  (nn.Linear without bias) on MFMA with fused
 * prologue / epilogue.  Replaces, per layer of unimatch/transformer.py: q/k/v projections (:58-60), merge +
 * LayerNorm (+ residual) (:137-138,:144), and the FFN  cat[source, message] -> 8C -> GELU -> C -> LayerNorm ->
 * + source (:141-144).  Same operand arithmetic as the attention kernels (`mode`).
 *   weights : um_weight_planes() turns W [N,K] fp32 into planes pre-scaled by 2^wshift (exact; keeps the fp16
 *             lo plane out of the subnormal range); pass the same wshift to um_linear_fwd.
 *   input   : exactly one of  a0 (fp32 [M,K])  |  a0 + a1 (fp32 [M,K/2] each: K-concatenation without the
 *             concatenated tensor)  |  a_planes ([NS][M][K]).
 *   epilogue: UM_EPI_PLANES       out = planes [NS][M][N]
 *             UM_EPI_LN           out = fp32 [M,N], N == 128: LayerNorm(gamma, beta, eps) (+ residual [M,N] if not NULL)
 *             UM_EPI_GELU_PLANES  out = planes of erf-GELU(C)
 * N must be a multiple of 128, K of 32 (64 with a1).
 * ------------------------------------------------------------------------------------------- */
#define UM_EPI_PLANES 0
#define UM_EPI_LN 1
#define UM_EPI_GELU_PLANES 2
size_t um_planes_bytes(long rows, int cols, int mode);
int um_weight_planes(const float* w, void* planes, int n, int k, int wshift, int mode, void* stream);
int um_linear_fwd(const float* a0, const float* a1, const void* a_planes, const void* w_planes,
                  int m, int n, int k, int wshift, int epilogue, void* out,
                  const float* gamma, const float* beta, const float* residual, float eps,
                  int mode, void* stream);

/* nn.Linear WITH bias -- the propagation layer's q / k projections (unimatch/attention.py:196-205 global, :229-232 local):
 *     C = (A . W^T) * out_mul + bias * bias_mul
 * input: exactly one of a0 (fp32 [M,K]) | a_planes ([NS][M][K]);  output: exactly one of out_planes ([NS][M][N], feeds
 * um_prop_global_attn_planes) | out_f32 ([M,N], feeds um_prop_local_attn).  w_planes / wshift as for um_linear_fwd; bias: fp32
 * [N], 16-byte aligned.  With A already scaled by s (planes carrying um_global_corr_plane_scale()), out_mul = 1 and
 * bias_mul = s give s * (W a + b). */
int um_linear_bias_fwd(const float* a0, const void* a_planes, const void* w_planes, const float* bias, int m, int n, int k,
                       int wshift, float out_mul, float bias_mul, void* out_planes, float* out_f32, int mode, void* stream);

/* Whole FFN of a Transformer layer in ONE kernel:
 *     out = x + LayerNorm( W2 . gelu( W1 . [x | y] ) )          (unimatch/transformer.py:141-144, mlp :44-50)
 * x (source, also the residual) and y (message): fp32 [M,128]; W1 [hidden, 256] and W2 [128, hidden] as
 * um_weight_planes() planes with the same wshift; gamma/beta/eps: the layer's norm2.  The [M, hidden]
 * activations stay on chip (the two-launch form um_linear_fwd(GELU_PLANES) + um_linear_fwd(LN) writes and reads them
 * through HBM).  hidden: multiple of 32, >= 64.  out: fp32 [M,128], may not alias x or y. */
int um_ffn_fwd(const float* x, const float* y, const void* w1_planes, const void* w2_planes, int m, int hidden,
               int wshift, const float* gamma, const float* beta, float eps, float* out, int mode, void* stream);
/* The same with an optional workspace of um_ffn_split_workspace_bytes(m, hidden) bytes that are ZERO before the first launch
 * (the kernel leaves them zero; one workspace serves one launch at a time).  With it a launch of few token tiles (batch 1:
 * 35 - 96 workgroups on 256 CUs, each walking all hidden slices) gives every tile to 2 or 4 neighbouring workgroups, each on
 * its share of the hidden units; the last one to finish sums the partial outputs (in part order) before LayerNorm.  The byte
 * count is 0 for launches that are not split. */
size_t um_ffn_split_workspace_bytes(int m, int hidden);
int um_ffn_ws_fwd(const float* x, const float* y, const void* w1_planes, const void* w2_planes, int m, int hidden,
                  int wshift, const float* gamma, const float* beta, float eps, float* out, int mode, void* workspace,
                  size_t workspace_bytes, void* stream);

/* The key / value projections of BOTH layers of a Transformer block (unimatch/transformer.py:58-60: k_proj / v_proj of the block's
 * self_attn and of its cross_attn_ffn, four bias-free 128 x 128 Linears of the token stream as it enters the block) in ONE launch
 * (round 4; two um_linear_fwd launches before):  x fp32 [m][128]  ->  out_planes [NS][4][m][128], the attention kernels' operand
 * planes in blocked form: projection j (0 k_self, 1 v_self, 2 k_cross, 3 v_cross) is the contiguous [m][128] tensor at element
 * offset j * m * 128 of every plane (plane stride 4 * m * 128, row stride 128: what um_window_attn_qproj_merge_fwd takes as
 * k_planes / v_planes + ldkv + kv_plane_stride).  wc_planes = um_weight_planes of the packed [256][256] fp32 matrix
 *     Wc[32 c + r][0:128] = W4[32 c + r][:],   Wc[32 c + r][128:256] = W4[256 + 32 c + (r ^ 16)][:],   c = 0..7, r = 0..31,
 * W4 = the four weights stacked [512][128] (unimatch_amd/ops.py::kv4_weight_planes builds it). */
int um_kv4_fwd(const float* x, const void* wc_planes, int m, int wshift, void* out_planes, int mode, void* stream);
/* um_ffn_ws_fwd of block i AND um_kv4_fwd of block i + 1 on its result, from ONE launch (closed in round 4):
 * every workgroup hands the 128-token tile it has just normalised to the k | v projection in its epilogue, so the next block's
 * keys / values (kv_planes, blocked [NS][4][m][128]) leave the FFN kernel directly and `out` is not read back.  Launches small
 * enough for the hidden split (um_ffn_split_workspace_bytes > 0) run the two kernels back to back inside the call. */
int um_ffn_kv_fwd(const float* x, const float* y, const void* w1_planes, const void* w2_planes, int m, int hidden, int wshift,
                  const float* gamma, const float* beta, float eps, float* out, const void* wc_planes, void* kv_planes, int mode,
                  void* workspace, size_t workspace_bytes, void* stream);
/* um_ffn_ws_fwd AND the operand planes of its result from ONE launch: out_planes [NS][m][128] is bit for bit
 * um_weight_planes(out, out_planes, m, 128, 0, mode) -- the hi | lo split of `out` at scale 1 -- written by the store loop that
 * writes `out`.  With the k | v projections folded into the query and merge weights (q' = Wk^T Wq, merge' = Wm Wv: single head,
 * bias-free, nothing non-linear between projection and attention) the token stream itself is the key / value operand of the next
 * block's two attention launches.  Launches small enough for the hidden split run the format pass as a second launch inside the call. */
int um_ffn_planes_fwd(const float* x, const float* y, const void* w1_planes, const void* w2_planes, int m, int hidden, int wshift,
                      const float* gamma, const float* beta, float eps, float* out, void* out_planes, int mode, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Convolutions either side of the matching path, NHWC, on the matrix cores with the same
 * operand arithmetic as everything else (`mode`): nn.Conv2d of unimatch/reg_refine.py:6-119 (3x3, 1x1, 1x5, 5x1, 7x7)
 * and unimatch/backbone.py:7-133 (3x3 at stride 1/2, 1x1 projections), dilation 1, groups 1.
 *   a_planes : activations as operand planes [NS][batch*hi*wi + 1][cin], NHWC, whose LAST row is all zeros (taps outside
 *              the image read it).  Written by um_nhwc_instance_norm / um_nchw_to_nhwc.  cin: multiple of 32.
 *   w_planes : um_weight_planes() of the weight permuted to [cout][kh][kw][cin] (n = cout, k = kh*kw*cin), same wshift.
 *   out      : fp32 [batch*ho*wo][cout] (NHWC), ho = (hi + 2 pad_h - kh) / stride + 1; + bias[cout] if not NULL (16-byte
 *              aligned); ReLU if relu.
 * ------------------------------------------------------------------------------------------- */
int um_conv2d_fwd(const void* a_planes, const void* w_planes, const float* bias, float* out, float* stats_out, int batch,
                  int hi, int wi, int cin, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int relu, int wshift,
                  int mode, void* stream);
/* General form.  The input planes are a column slice [a_coff, a_coff + cin) of a buffer [NS][a_rows][a_ld] whose LAST row
 * (a_rows - 1 >= batch*hi*wi) is all zeros; the result goes to fp32 `out` [.][out_ld] at column out_coff and / or, as operand
 * planes, to `out_planes` [NS][outp_rows][outp_ld] at column outp_coff -- so a chain of convolutions needs no fp32 round trip
 * and channel concatenations (torch.cat of reg_refine.py:33-35, 50-53, 62-66) are column offsets.  act: 0 none, 1 ReLU,
 * 2 sigmoid, 3 tanh (the GRU gates of reg_refine.py:55-76).  Leading dimensions / offsets: multiples of 8 (input) / 4 (output). */
int um_conv2d_ex(const void* a_planes, int a_ld, int a_coff, long a_rows, const void* w_planes, const float* bias, float* out,
                 int out_ld, int out_coff, void* out_planes, int outp_ld, int outp_coff, long outp_rows, float* stats_out,
                 int batch, int hi, int wi, int cin, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int act,
                 int wshift, int mode, void* stream);
/* The two convolutions of a SepConvGRU half (unimatch/reg_refine.py:66-74) with the gate arithmetic in the epilogue.
 *   gate 1: weights = [z ; r] stacked (2*channels outputs), sigmoid; z -> z_out [.][z_out_ld] (fp32), and r * hidden is written
 *           as operand planes at (out_planes, outp_ld, outp_coff) -- the q convolution's input;
 *   gate 2: weights = q (channels outputs), tanh; hidden <- (1 - z) * hidden + z * q in place (fp32 [.][channels], z = z[.][z_ld])
 *           and as operand planes (the next convolution's input).
 * Input slice / stride 1 / padding as um_conv2d_ex. */
int um_conv2d_gru_fwd(int gate, const void* a_planes, int a_ld, int a_coff, long a_rows, const void* w_planes, const float* bias,
                      float* hidden, const float* z, int z_ld, float* z_out, int z_out_ld, void* out_planes, int outp_ld,
                      int outp_coff, long outp_rows, int batch, int hi, int wi, int cin, int channels, int kh, int kw, int pad_h,
                      int pad_w, int wshift, int mode, void* stream);
/* The same with a per-pixel addend (fp32 [rows][addend_ld]; column = output channel of the convolution: 2 * channels for gate 1,
 * channels for gate 2), added to the scaled accumulator (+ bias) BEFORE the gate's activation.  A convolution is linear in its input
 * channels: the refinement loop (unimatch/unimatch.py:315-331) restarts its hidden state from the same net0 and feeds the same
 * context features `inp` in every iteration, so their share of every gate convolution is computed ONCE per scale (um_conv2d_ex,
 * no activation) and the per-iteration convolutions only read the channels that change (round 4; unimatch_amd/refine_nhwc.py).
 * gate 2 (v211): `z_out`, when non-null, receives the NEW hidden state (fp32 [rows][z_out_ld >= channels]) and `hidden` is only read --
 * the loop's first q convolution reads net0 and writes the working state, so net0 is never copied (null: `hidden` updated in place). */
int um_conv2d_gru_add_fwd(int gate, const void* a_planes, int a_ld, int a_coff, long a_rows, const void* w_planes, const float* bias,
                          const float* addend, int addend_ld, float* hidden, const float* z, int z_ld, float* z_out, int z_out_ld,
                          void* out_planes, int outp_ld, int outp_coff, long outp_rows, int batch, int hi, int wi, int cin,
                          int channels, int kh, int kw, int pad_h, int pad_w, int wshift, int mode, void* stream);
/* um_conv2d_fwd (no activation, no statistics) with an fp32 addend in the epilogue: out = (acc * 2^-wshift + bias) + addend -- the value
 * the plain launch stores, then ONE fp32 add of its own (nothing is contracted across the two), so the result is bit for bit
 * um_conv2d_fwd's plus the addend.  addend: 16-byte aligned, addend_ld >= cout, a multiple of 4.  addend_period = 0: one row per output
 * pixel, [batch*ho*wo][addend_ld]; addend_period = 1: ONE table [ho*wo][addend_ld] that serves every image (row = pixel inside the image):
 * the Transformer's position table (unimatch/unimatch.py:139, feature_add_position) in the encoder's last convolution. */
int um_conv2d_addend_fwd(const void* a_planes, const void* w_planes, const float* bias, const float* addend, int addend_ld,
                         int addend_period, float* out, int batch, int hi, int wi, int cin, int cout, int kh, int kw, int stride,
                         int pad_h, int pad_w, int wshift, int mode, void* stream);
/* stats_out (optional): per output tile part (<= 128 pixels, in the order of the serving kernel's tiles) the (mean, pixel
 * count, sum of squared deviations) of every output channel, computed in the epilogue from the tile that is in LDS anyway.
 * um_conv_stats_parts() = parts per image for that geometry (the stem, um_conv7_fwd / um_stem_conv_fwd: kh = kw = 7,
 * stride 2, pad 3); the buffer holds um_conv_stats_bytes(batch, parts, cout) bytes; pass both to
 * um_nhwc_instance_norm(conv_stats, conv_stats_parts) and the normalisation skips its own statistics pass. */
int um_conv_stats_parts(int hi, int wi, int cout, int kh, int kw, int stride, int pad_h, int pad_w);
size_t um_conv_stats_bytes(int batch, int parts, int channels);

/* The encoder's 7x7 / stride-2 / pad-3 stem (unimatch/backbone.py:49; 3 input channels, no bias) on the same kernel, always
 * in the exact arithmetic.  image: fp32 NCHW [batch,3,h,w]; with `normalize` the reference's input normalisation
 * ((x / 255 - mean) / std, unimatch/unimatch.py:122-124) is applied while packing.  image_planes: scratch of
 * um_stem_planes_bytes() bytes (the zero-bordered NHWC-4 operand planes).  w_planes: um_weight_planes() of the weight
 * rearranged to [cout][7 ky][8 kx][4 ci] with zeros at kx = 7 and ci = 3 (n = cout, k = 224).  out: fp32 NHWC
 * [batch * ho * wo][cout], ho = (h - 1) / 2 + 1.  stats_out: as um_conv2d_fwd. */
size_t um_stem_planes_bytes(int batch, int h, int w);
/* General form: 7x7 / pad 3 convolution of an fp32 NCHW image with few channels (stride 2: <= 3 channels, packed 4 per pixel;
 * stride 1: <= 8 channels, packed 8 per pixel -- the motion encoder's flow branch, unimatch/reg_refine.py:13), outputs as
 * um_conv2d_ex.  w_planes: the weight rearranged to [cout][7 ky][8 kx][cpp] with zeros at kx = 7 and the missing channels
 * (k = 56 cpp).  mean3 / std3 are HOST arrays. */
size_t um_conv7_planes_bytes(int batch, int h, int w, int stride);
int um_conv7_fwd(const float* image, int channels, int normalize, const float* mean3, const float* std3, void* image_planes,
                 const void* w_planes, const float* bias, float* out, int out_ld, int out_coff, void* out_planes, int outp_ld,
                 int outp_coff, long outp_rows, float* stats_out, int batch, int h, int w, int cout, int stride, int act,
                 int wshift, void* stream);
int um_stem_conv_fwd(const float* image, int normalize, const float* mean3, const float* std3, void* image_planes,
                     const void* w_planes, float* out, float* stats_out, int batch, int h, int w, int cout, int wshift,
                     void* stream);

/* um_stem_conv_fwd of the batch [image0; image1] -- batch0 + batch1 images of one size in two tensors (the two images of every pair,
 * unimatch/unimatch.py:126 concatenates them) -- without the concatenation: the packing kernel picks its source by image index.
 * image_planes: um_stem_planes_bytes(batch0 + batch1, h, w).  Planes, launch, statistics and output are bit for bit those of
 * um_stem_conv_fwd on the concatenated batch. */
int um_stem_conv_pair_fwd(const float* image0, int batch0, const float* image1, int batch1, int normalize, const float* mean3,
                          const float* std3, void* image_planes, const void* w_planes, float* out, float* stats_out, int h, int w,
                          int cout, int wshift, void* stream);

/* nn.InstanceNorm2d (affine=False, biased variance) + ReLU (+ shortcut add + ReLU) of unimatch/backbone.py:7-36 in NHWC:
 *   y = x (normalize == 0) | (x - mean_{b,c}) * rsqrt(var_{b,c} + eps);  y = relu(y) if relu;  y = relu(shortcut + y) if
 * shortcut.  x, shortcut: fp32 [batch*pixels][channels]; alternatively (shortcut == NULL) shortcut_planes: the shortcut as
 * operand planes [NS][batch*pixels + 1][channels] (hi + lo is added) -- a residual block's identity shortcut is the planes
 * its first convolution read, so no fp32 copy of the block input has to exist.  Outputs (either may be NULL): operand planes
 * [NS][batch*pixels + 1][channels] including the zero row um_conv2d_fwd expects, and fp32 [batch*pixels][channels].
 * Statistics are deterministic (fixed reduction order, chunk-shifted sums merged in fp64).  channels: multiple of 8, <= 256. */
size_t um_nhwc_norm_workspace_bytes(int batch, int pixels, int channels);
int um_nhwc_instance_norm(const float* x, const float* shortcut, const void* shortcut_planes, void* planes_out, float* f32_out,
                          int batch, int pixels, int channels, float eps, int normalize, int relu, const float* conv_stats,
                          int conv_stats_parts, void* workspace, size_t workspace_bytes, int mode, void* stream);

/* The channel concatenation [map | tokens | zero pad] as operand planes in one launch (the upsampler head's input cat(flow, feature),
 * unimatch/unimatch.py:56-58).  map: fp32 NCHW [batch][map_channels][pixels], 1 <= map_channels <= 4; tokens: fp32
 * [batch*pixels][channels] (16-byte aligned, channels a multiple of 4, <= 256).  planes_out: [NS][batch*pixels + 1][cp], cp =
 * map_channels + channels rounded up to a multiple of 32: the map in columns 0 .. map_channels-1, the tokens behind it, zero columns
 * up to cp and the zero row -- bit for bit what um_nhwc_instance_norm(normalize = 0) writes for the fp32 concatenation. */
int um_nhwc_concat_planes(const float* map, const float* tokens, void* planes_out, int batch, int pixels, int map_channels, int channels,
                          int mode, void* stream);

/* um_nhwc_instance_norm whose fp32 `shortcut` is a projection shortcut's RAW convolution output: its own InstanceNorm (no ReLU,
 * unimatch/backbone.py:24-25) is computed in registers from sc_conv_stats / sc_conv_stats_parts (the per-tile statistics that
 * convolution left) -- the value a normalisation pass of its own would have stored and this one read back, bit for bit.  The other
 * arguments are um_nhwc_instance_norm's; normalize must be 1; workspace: um_nhwc_norm_sc_workspace_bytes(). */
size_t um_nhwc_norm_sc_workspace_bytes(int batch, int pixels, int channels);
int um_nhwc_instance_norm_sc(const float* x, const float* shortcut, const void* shortcut_planes, void* planes_out, float* f32_out,
                             int batch, int pixels, int channels, float eps, int normalize, int relu, const float* conv_stats,
                             int conv_stats_parts, void* workspace, size_t workspace_bytes, int mode, void* stream,
                             const float* sc_conv_stats, int sc_conv_stats_parts);

/* The statistics step of um_nhwc_instance_norm on its own: per-part statistics of a convolution's epilogue (conv_stats,
 * conv_stats_parts = um_conv_stats_parts() of that convolution) -> stats_out fp32 [batch][2][channels] = (mean, 1 / sqrt(var + eps)),
 * the same kernel and the same bits um_nhwc_instance_norm(conv_stats) computes internally. */
int um_nhwc_stats_finalize(const float* conv_stats, int conv_stats_parts, float* stats_out, int batch, int pixels, int channels,
                           float eps, void* stream);
/* Normalise on load: um_conv2d_fwd whose input is not operand planes but the PRODUCING convolution's fp32 output
 * x [batch*hi*wi][cin] (16-byte aligned) and its statistics norm_stats [batch][2][cin] (um_nhwc_stats_finalize); the patch kernel
 * computes relu?((x - mean) * rstd) and the hi | lo split while it stages the operand, in um_nhwc_instance_norm's arithmetic:
 * output and stats_out are bit-identical to um_nhwc_instance_norm(planes_out) -> um_conv2d_fwd, without the normalisation's pass
 * over memory (the middle InstanceNorm of a residual block, unimatch/backbone.py:27-31).  `relu`: on the output, as um_conv2d_fwd.
 * Served for the geometries um_conv2d_norm_supported() returns 1 for (3x3 / stride 1 / pad 1 maps the 2-D patch kernel takes, at
 * the tile widths where the path measured faster) -- a pure function of its arguments; any other geometry is an error (-2). */
int um_conv2d_norm_supported(int hi, int wi, int cin, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int mode);
int um_conv2d_norm_fwd(const float* x, const float* norm_stats, int norm_relu, const void* w_planes, const float* bias, float* out,
                       float* stats_out, int batch, int hi, int wi, int cin, int cout, int kh, int kw, int stride, int pad_h,
                       int pad_w, int relu, int wshift, int mode, void* stream);

/* A transition block's entry in one launch (conv_entry_kernel, the generic kernel's entry variant).  The block input
 * X = relu(norm(u) + S) of a stride-2 residual block (unimatch/backbone.py:7-36) is read only by that block's 3x3 / stride 2 / pad 1
 * convolution and its 1x1 / stride 2 projection, which samples the centre tap of the 3x3 window.  u: the previous block's conv2 output,
 * fp32 [batch*hi*wi][cin]; ustats: its statistics [batch][2][cin] (um_nhwc_stats_finalize); s_planes: that block's shortcut as operand
 * planes [NS][batch*hi*wi + 1][cin].  X is built while the operand is staged, in um_nhwc_instance_norm's arithmetic, and never
 * written; out_t = conv3x3(X) (w_planes, no bias) and out_d = conv1x1(X) + bias2 (w2_planes), fp32 [batch*ho*wo][cout], each with its
 * per-tile statistics (stats_t / stats_d, um_conv_stats_parts() of either geometry: the same number) -- bit-identical to
 * um_nhwc_instance_norm(u, shortcut_planes = S, relu) -> um_conv2d_fwd(3x3) and um_conv2d_fwd(1x1, bias).  Counted once as
 * UM_V_CONV_GENERIC.  Served for the geometries um_conv2d_entry_supported() returns 1 for (3x3 / stride 2 / pad 1, cin a multiple
 * of 32 and <= 128, at the tile widths where the path measured faster) -- a pure function of its arguments; any other geometry is
 * an error (-2) and nothing is launched. */
int um_conv2d_entry_supported(int hi, int wi, int cin, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int mode);
int um_conv2d_entry_fwd(const float* u, const float* ustats, const void* s_planes, const void* w_planes, const void* w2_planes,
                        const float* bias2, float* out_t, float* out_d, float* stats_t, float* stats_d, int batch, int hi, int wi,
                        int cin, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int wshift, int mode, void* stream);

/* Channels-last element-wise helpers of the refinement block (SepConvGRU, unimatch/reg_refine.py:55-76); every result is
 * written as operand planes into columns [coff, coff + channels) of a buffer [NS = 2][plane_rows][ld]:
 *   mode 0  planes = src[rows][src_ld] (first `channels` columns)                      -- column scatter (flow, hidden state)
 *   mode 1  planes = r * h,   r = zr[rows][2C] columns C..2C,  h = hbuf[rows][C]
 *   mode 2  h <- (1 - z) * h + z * q  (z = zr columns 0..C, q = src), written back to hbuf and (if planes_out) as planes. */
int um_nhwc_gate(int mode, const float* src, int src_ld, const float* zr, float* hbuf, void* planes_out, int ld, int coff,
                 long plane_rows, long rows, int channels, void* stream);

/* fp32 NCHW [batch][channels][pixels] (the output of a MIOpen convolution) -> NHWC operand planes (with the zero row)
 * and / or fp32 NHWC.  channels: multiple of 8, <= 256. */
int um_nchw_to_nhwc(const float* x, void* planes_out, float* f32_out, int batch, int channels, int pixels, int mode,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * All-pairs correlation + softmax + expected coordinate (flow).
 * Replaces unimatch/matching.py:7-36 global_correlation_softmax (the [B,L,L] correlation and
 * probability tensors are never formed).  f0, f1: [B, h*w, C].  flow: [B or 2B, 2, h, w]
 * (bidir != 0 appends the backward flow, matching.py:23-27).
 * ------------------------------------------------------------------------------------------- */
size_t um_global_corr_workspace_bytes(int batch, int tokens, int channels, int mode);
int um_global_corr_softmax_flow(const float* f0, const float* f1, float* flow,
                                int batch, int h, int w, int channels, int bidir,
                                int mode, void* workspace, size_t workspace_bytes, void* stream);

/* Per-scanline W x W correlation, targets right of the query masked, disparity = x - E[x'].
 * Replaces unimatch/matching.py:126-151 global_correlation_softmax_stereo.  disp: [B, 1, h, w]. */
int um_global_corr_softmax_stereo(const float* f0, const float* f1, float* disp,
                                  int batch, int h, int w, int channels,
                                  int mode, void* workspace, size_t workspace_bytes, void* stream);

/* Global self-attention propagation  softmax(q k^T / sqrt(C)) value.
 * Replaces the attention core of unimatch/attention.py:196-213 SelfAttnPropagation.forward
 * (q/k projections stay with the caller).  q, k: [B, h*w, C]; value, out: [B, V, h, w], V in {1,2}. */
int um_prop_global_attn(const float* q, const float* k, const float* value, float* out,
                        int batch, int h, int w, int channels, int value_channels,
                        int mode, void* workspace, size_t workspace_bytes, void* stream);
/* The same on operands that are already MFMA planes ([NS][batch*h*w][128]) carrying um_global_corr_plane_scale(channels) on
 * both q and k (= sqrt(log2(e) / sqrt(C)): the kernels take the softmax logit in log2 units straight from the MFMA) -- the
 * output of um_linear_bias_fwd(out_planes).  Workspace as um_global_corr_workspace_bytes(). */
float um_global_corr_plane_scale(int channels);
int um_prop_global_attn_planes(const void* q_planes, const void* k_planes, const float* value, float* out, int batch, int h,
                               int w, int channels, int value_channels, int mode, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Matching confidence: statistics of every row of the matching distribution `prob` that
 * global_correlation_softmax (unimatch/matching.py:7-36) and global_correlation_softmax_stereo
 * (matching.py:126-151) return next to the flow / disparity, without forming it (csrc/match_stats.hip).
 * With p_ij = softmax_j(q_i . k_j / sqrt(C)) over all keys (flow) or over the keys x' <= x of the query's
 * scanline (stereo), per query i:
 *   stats[:, 0] max_prob  max_j p_ij
 *   stats[:, 1] entropy   -sum_j p_ij ln p_ij  (nats, 0 ln 0 = 0)
 *   stats[:, 2] variance  sum_j p_ij |g_j - mu_i|^2, mu_i = sum_j p_ij g_j, g = pixel coordinates (flow: 2-D; stereo: x), >= 0
 *   best                  argmax_j p_ij: the key's token index y*w + x (flow) or its column x' (stereo); ties go to the lowest index
 *   mean (may be NULL)    mu_i - g_i: the flow (2 channels) / minus the disparity (1 channel) of the entry points above
 * A stereo query at x = 0 has one key: exactly (1, 0, 0).  f0, f1: [B, h*w, C].  stats [B', 3, h, w], best [B', h, w] int32,
 * mean [B', 2 or 1, h, w]; bidir (flow only) appends the f1 -> f0 direction, B' = 2B; stereo != 0 excludes bidir.
 * Every element of stats, best and mean is written; nothing is read beyond f0, f1 and the workspace.
 *
 * um_match_mutual: mutual[b, i] = 1 iff i' = best_bwd[b, best_fwd[b, i]] lies within `radius` feature pixels of i in both x
 * and y (radius 0: exact mutual nearest neighbours); an index outside [0, h*w) is no match.  best_*: [B, h, w] token indices.
 * ------------------------------------------------------------------------------------------- */
size_t um_global_match_stats_workspace_bytes(int batch, int tokens, int channels, int mode);
int um_global_match_stats(const float* f0, const float* f1, float* stats, int* best, float* mean,
                          int batch, int h, int w, int channels, int bidir, int stereo,
                          int mode, void* workspace, size_t workspace_bytes, void* stream);
int um_match_mutual(const int* best_fwd, const int* best_bwd, unsigned char* mutual, int batch, int h, int w, int radius,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Local-window kernels (fp32 VALU, wavefront-shuffle reductions; `mode` does not apply).
 * ------------------------------------------------------------------------------------------- */

/* (2r+1)^2 (or 2r+1 when one_d) integer-offset correlation, out-of-image taps -> -1e9, softmax,
 * expected offset.  Replaces unimatch/matching.py:39-83 local_correlation_softmax (flow [B,2,h,w])
 * and :154-200 local_correlation_softmax_stereo (one_d != 0: returns -flow_x as [B,1,h,w]). */
int um_local_corr_softmax(const float* f0, const float* f1, float* out,
                          int batch, int h, int w, int channels, int radius, int one_d, void* stream);

/* Local cost volume at flow-displaced positions: out[k,p] = f0(p) . bilinear(f1, p + d_k + flow(p)) / sqrt(C),
 * zeros outside.  Replaces unimatch/matching.py:86-123 local_correlation_with_flow (dilation 1).
 * flow: [B, 2, h, w]; cost: [B, (2r+1)^2, h, w]. */
int um_local_corr_with_flow(const float* f0, const float* f1, const float* flow, float* cost,
                            int batch, int h, int w, int channels, int radius, void* stream);
/* The same with the reference's `dilation` argument (matching.py:86-91): taps at p + dilation * d_k + flow(p).  dilation = 1 is
 * um_local_corr_with_flow; larger dilations take a plain four-corner gather per tap (no caller of the reference uses them). */
int um_local_corr_with_flow_dilated(const float* f0, const float* f1, const float* flow, float* cost,
                                    int batch, int h, int w, int channels, int radius, int dilation, void* stream);
/* Same cost volume written channels-last as the operand planes of the motion encoder's 1x1 convolution
 * (unimatch/reg_refine.py:11,20): planes_out [2][plane_rows][ld], pixel row = (2r+1)^2 taps then zeros up to ld; the fp32
 * [B, taps, h, w] volume is never formed ("K4 fused into convc1"). */
int um_local_corr_with_flow_planes(const float* f0, const float* f1, const float* flow, void* planes_out, int ld, long plane_rows,
                                   int batch, int h, int w, int channels, int radius, void* stream);

/* The same cost volume on the matrix cores for locally coherent flow (csrc/local_corr_mfma.hip): an 8 x 4 pixel tile whose
 * 10 x 10 integer neighbourhoods fit a 32 x 24 window of f1 gets every dot product from one 32 x 32 x 128 MFMA product per
 * window row; other tiles (motion boundaries) take the pixel-at-a-time path inside the same kernel.  The refinement loop
 * (unimatch/unimatch.py:315-331) calls matching.py:86-123 with the SAME feature0 / feature1 in every iteration, so their fp16
 * hi | lo operand planes are built once per scale:
 *   um_local_corr_feat_planes_bytes(...)                bytes of `feat_planes`
 *   um_local_corr_feat_planes(f0, f1, feat_planes, ...) fill it ([B, h*w, 128] fp32 tokens in)
 *   um_local_corr_with_flow_feat_supported(...)         1 for radius 4 on maps of whole 8 x 4 tiles
 *   um_local_corr_with_flow_feat(...)                   exactly one of `cost` ([B, 81, h, w] fp32) and `planes_out` (as
 *                                                       um_local_corr_with_flow_planes) non-null; flags bit 0 = every tile on
 *                                                       the pixel-at-a-time path, bit 1 = natural 8 x 4 tiles only (A/B timing).
 *   Where more than a quarter of a launch's natural tiles have incoherent flow (no common 32 x 24 window) the pixels are grouped by
 *   the 16 x 8 cell of f1 they sample (counting sort on the device, scratch inside `feat_planes`) and the groups run on the matrix
 *   cores: the choice is a function of the call's flow alone and the result is bitwise reproducible (profiles/r05_k4_target_order.txt). */
size_t um_local_corr_feat_planes_bytes(int batch, int h, int w, int channels);
int um_local_corr_feat_planes(const float* f0, const float* f1, void* feat_planes, int batch, int h, int w, int channels,
                              void* stream);
int um_local_corr_with_flow_feat_supported(int h, int w, int channels, int radius);
/* um_local_corr_softmax (2-D, radius 4, maps of whole 8 x 4 tiles) on the same kernel: every pixel's 81 taps are its own 9 x 9
 * neighbourhood, so the whole map takes the matrix-core path.  workspace: um_local_corr_feat_planes_bytes(). */
int um_local_corr_softmax_mfma(const float* f0, const float* f1, float* out, int batch, int h, int w, int channels, int radius,
                               void* workspace, size_t workspace_bytes, void* stream);
int um_local_corr_with_flow_feat(const float* f0, const float* f1, const void* feat_planes, const float* flow, float* cost,
                                 void* planes_out, int ld, long plane_rows, int batch, int h, int w, int channels, int radius,
                                 int flags, unsigned* stats /* optional device [2]: += tiles on the product / pixel path */,
                                 void* stream);

/* (2r+1)^2 local self-attention propagation with zero-padded keys/values (out-of-image neighbours
 * have logit 0, value 0 and take part in the softmax).
 * Replaces the core of unimatch/attention.py:217-253 forward_local_window_attn. */
int um_prop_local_attn(const float* q, const float* k, const float* value, float* out,
                       int batch, int h, int w, int channels, int value_channels, int radius,
                       void* stream);

/* Plane-sweep depth correlation + softmax over D inverse-depth candidates + soft-argmin / argmax.
 * Replaces unimatch/matching.py:203-282 correlation_softmax_depth + warp_with_pose_depth_candidates.
 * cam: [B, 30] fp32 per-sample camera constants, row major:  K^-1 (9) | R (9) | t (3) | K (9), with K the
 * intrinsics already divided by the feature stride (unimatch/unimatch.py:147-150) and [R|t] the relative
 * pose; the kernel applies them in the reference's order (back-project, rotate, scale by depth, translate,
 * project, clamp z >= 1e-3).  candidates: [D] inverse depths.  out: [B, 1, h, w] inverse depth. */
int um_depth_corr_softmax(const float* f0, const float* f1, const float* cam, const float* candidates,
                          float* out, int batch, int h, int w, int channels, int num_candidates,
                          int from_argmax, void* stream);

/* um_depth_corr_softmax plus the statistics of the distribution it reduces, in the same launch.  The reference returns
 * that distribution -- correlation_softmax_depth gives (depth, match_prob [B, D, h, w]), matching.py:227 -- and the plane
 * sweep here never forms it.  f0 .. out and from_argmax as above (same kernels, same arithmetic for `out`).  With
 * p_j = softmax_j(logit_j) over the D candidates c_j of a pixel:
 *   stats [B, 4, h, w] fp32:  0 max_prob = max_j p_j | 1 entropy = -sum p ln p (nats, 0 .. ln D) |
 *                             2 variance = sum p_j (c_j - mu)^2 about mu = sum p_j c_j (inverse depth squared) |
 *                             3 peak_mass = sum of p_j over |j - best| <= peak_radius (radius 0: max_prob)
 *   index [B, 2, h, w] int32: 0 best = the first j attaining the maximum logit (what from_argmax reads out) |
 *                             1 in_view = candidates with a bilinear corner inside the image (0: every logit is exactly 0,
 *                               the distribution is uniform)
 * stats or index may be NULL: that output is not written.  Errors (negative, nothing launched): a null f0 / f1 / cam /
 * candidates / out, channels != 128, num_candidates outside 1 .. 128, peak_radius < 0. */
int um_depth_corr_softmax_stats(const float* f0, const float* f1, const float* cam, const float* candidates,
                                float* out, float* stats, int* index,
                                int batch, int h, int w, int channels, int num_candidates,
                                int from_argmax, int peak_radius, void* stream);

/* The plane sweep with several source views voting in ONE cost volume before the softmax (csrc/depth_multi.hip).  Sources
 * s = 0 .. S-1 share the reference pixel and the candidates c_j.  For a source that is on, l_sj is exactly the logit
 * um_depth_corr_softmax forms for (f0_s, f1_s, cam_s) and v_sj = 1 when candidate j has a bilinear corner inside the image of
 * source s (x0 in [-1, w-1] and y0 in [-1, h-1]).  Fused:
 *   n_j = sum_s v_sj,   l_j = (sum_s v_sj l_sj) / max(1, n_j),   p = softmax_j l_j
 * -- a mean over the sources that SEE the candidate, which keeps the logits at the scale the softmax was trained at.  This is an
 * UNLEARNED extension: the weights are trained on two views.  out, stats and index are those of um_depth_corr_softmax_stats taken
 * on p (best = first arg-max of l, in_view = candidates with n_j >= 1).  One source given 2 or 4 times gives bit for bit the S = 1
 * result (2l/2 and 4l/4 are exact), and S = 1 gives bit for bit the result of um_depth_corr_softmax_stats.
 *   f0, f1 [S, B, h*w, 128] (each source has its own f0_s: after cross-attention the reference tokens depend on the partner view),
 *   cam [S, B, 30], use [S, B] bytes (0: the source is off for that sample and is never read) or NULL = all on,
 *   out [B, 1, h, w], stats [B, 4, h, w] or NULL, index [B, 2, h, w] or NULL.  Source-major: S = 1 is the two-view layout.
 * `use` lives on the device and is not inspected by the host: a sample whose sources are all off gets the uniform distribution
 * (every logit 0, in_view 0).  Errors (negative, nothing launched): a null f0 / f1 / cam / candidates / out, channels != 128,
 * num_candidates outside 1 .. 128, sources outside 1 .. 8, peak_radius < 0. */
int um_depth_corr_softmax_multi(const float* f0, const float* f1, const float* cam, const unsigned char* use,
                                const float* candidates, float* out, float* stats, int* index,
                                int sources, int batch, int h, int w, int channels, int num_candidates,
                                int from_argmax, int peak_radius, void* stream);

/* um_depth_corr_softmax_multi on operands that are ROWS of other tensors, named by a table instead of copied into the source-major
 * layout: the same fusion rule, arithmetic, outputs and kernel forms, bit for bit the contiguous entry's result on the same operands.
 *   segments      HOST array of num_segments (1 .. 4) device pointers, segment i = [segment_rows[i], h*w, 128] fp32;
 *   segment_rows  HOST int array.  A token row index addresses the concatenation of the segments in order.  Both arrays are read
 *                 before the call returns; the table reaches the kernel by value in its arguments.
 *   cam [cam_rows, 30], candidates [D],
 *   rows [S, B, 3] int32 on the DEVICE = f0 row | f1 row | cam row of source s for sample b.  The host does not inspect it.  A source
 *                 any of whose three indices is negative or out of range (>= the segments' total rows, >= cam_rows for the cam row)
 *                 is OFF for that sample and is never read -- the `use` of the contiguous entry, and what keeps a bad table from
 *                 reading out of bounds.  A sample whose sources are all off gets the uniform distribution, in_view 0.
 *   out, stats, index, from_argmax, peak_radius, stream: as above.
 * Errors (negative, nothing launched): a null segments / segment_rows / cam / rows / candidates / out, a null segment pointer or
 * segment_rows[i] <= 0, num_segments outside 1 .. 4, cam_rows <= 0, channels != 128, num_candidates outside 1 .. 128, sources outside
 * 1 .. 8, peak_radius < 0. */
int um_depth_corr_softmax_multi_rows(const float* const* segments, const int* segment_rows, int num_segments,
                                     const float* cam, int cam_rows, const int* rows, const float* candidates,
                                     float* out, float* stats, int* index, int sources, int batch, int h, int w, int channels,
                                     int num_candidates, int from_argmax, int peak_radius, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RAFT convex upsampling (SURVEY.md 8(f) "next" row): softmax over the 9 neighbours of each of factor^2 sub-pixels,
 * weighted sum of the 3x3 (zero padded) neighbourhood of mult * flow, pixel shuffle.  Replaces
 * upsample_flow_with_mask (unimatch/utils.py:134-152).  flow: [B, V, h, w] (V = 1 | 2), mask: [B, 9*factor^2, h, w]
 * (channel = k*factor^2 + fy*factor + fx), up: [B, V, factor*h, factor*w]; mult = 1 if is_depth else factor;
 * factor 4 or 8.
 * ------------------------------------------------------------------------------------------- */
int um_convex_upsample(const float* flow, const float* mask, float* up, int batch, int channels, int h, int w,
                       int factor, int is_depth, int mask_nhwc, void* stream);
/* mask_nhwc: the mask is [batch][h*w][9*factor^2] (the output of um_conv2d_fwd) instead of NCHW. */

/* flow_warp (unimatch/geometry.py:41-72, call sites unimatch/unimatch.py:166-168): bilinear warp of a token-major feature
 * [batch][h*w][channels] by flow [batch][2][h][w] (x, y), zeros outside, align_corners -> out_tokens, same layout.
 * SURVEY.md 8(f) rank 2. */
int um_flow_warp(const float* feature_tokens, const float* flow, float* out_tokens, int batch, int h, int w, int channels,
                 void* stream);

/* Video post-processing (csrc/video.hip), applied to a batch of predicted flows; both memory-bound, no state between calls.
 *   um_fwd_bwd_occlusion  forward_backward_consistency_check (unimatch/geometry.py:75-96) in one launch: fwd, bwd [B,2,H,W] fp32 ->
 *                         occ_fwd, occ_bwd [B,H,W] fp32 in {0, 1}.  Per pixel p and direction: the other flow sampled at p + flow(p)
 *                         (bilinear, zeros outside, grid_sample align_corners=True with the reference's normalise / un-normalise
 *                         round trip), occluded where |flow + warped| > alpha (|fwd| + |bwd|) + beta.  H, W >= 2.
 *   um_flow_to_rgb        flow_to_image (utils/flow_viz.py:231-254) per image: flow [B,2,H,W] fp32 -> rgb [B,H,W,3] uint8.  Unknown
 *                         flow (|u| or |v| > 1e7) is black; each image is normalised by its OWN maximum |flow| plus float64 eps (-1
 *                         when that maximum is NaN, as max(-1, np.max(rad)) gives); Middlebury wheel of 55 hues, float64 from the
 *                         normalisation on.  Two launches (partial maxima into `workspace`, then colour): no atomics, no counters, every
 *                         workspace slot is rewritten by each call.  workspace >= um_flow_to_rgb_workspace_bytes(batch, h, w) (0 for
 *                         bad sizes). */
int um_fwd_bwd_occlusion(const float* fwd, const float* bwd, float* occ_fwd, float* occ_bwd, int batch, int h, int w, float alpha,
                         float beta, void* stream);
size_t um_flow_to_rgb_workspace_bytes(int batch, int h, int w);
int um_flow_to_rgb(const float* flow, unsigned char* rgb, int batch, int h, int w, void* workspace, size_t ws_bytes, void* stream);

/* Point tracks (csrc/video.hip): follow n points through the `pairs` consecutive flows of a sequence in one launch, one thread per
 * track with its position and alive flag in registers.  flow [pairs,2,h,w] fp32 (pair t maps frame t to frame t + 1), occ
 * [pairs,h,w] fp32 (1 = occluded, the occ_fwd of um_fwd_bwd_occlusion) or NULL.  A track is (x, y) in pixel coordinates of the current
 * frame; inside(x, y) is 0 <= x <= w - 1 and 0 <= y <= h - 1 (false for a NaN).  It starts at pos_in[i] ([n,2] fp32), or with
 * pos_in == NULL at point i = ((i % gw) * grid_stride, (i / gw) * grid_stride) of the grid gw = ceil(w / grid_stride), gh =
 * ceil(h / grid_stride), n == gw * gh (grid_stride is ignored when pos_in is given); alive = alive_in[i] (NULL: all) && inside.  Step t of
 * an alive track: (u, v) = bilinear sample of flow t at (x, y), o = bilinear sample of occ t at the same (old) position (pixel
 * coordinates, taps outside the frame add zero); x += u, y += v; alive = inside(x, y) && !(o >= 0.5).  A track that is not alive keeps
 * its position -- the one of the step that lost it -- and never recovers.  Writes tracks [pairs,n,2] fp32 (8-byte aligned) and visible
 * [pairs,n] bytes in {0, 1} after every step; the last rows are the state to continue from (as pos_in / alive_in of the next call).
 * With grid_stride 1, tracks[t] - grid is the dense long-range flow F(0 -> t+1) = F(0 -> t) + flow_warp(F(t -> t+1), F(0 -> t))
 * (unimatch/geometry.py:41-72).  h, w >= 2; h * w, n, pairs * n, pairs * h * w <= 2^30.  No workspace, no atomics, no state. */
int um_flow_chain(const float* flow, const float* occ, const float* pos_in, const unsigned char* alive_in, float* tracks,
                  unsigned char* visible, int pairs, int h, int w, int n, int grid_stride, void* stream);

/* Evaluation metrics (csrc/metrics.hip): the statistics of the reference's validation loops, reduced on the device.  `pred` is the
 * batch as the model returned it, STILL PADDED ([B,2,hp,wp] flow, [B,hp,wp] disparity / depth); ground truth and masks are
 * [B,(2,)h,w] fp32, and ground-truth pixel (y, x) is compared with pred pixel (y + top, x + left): the InputPadder's crop, read in
 * place.  0 <= top, top + h <= hp, 0 <= left, left + w <= wp, else UM_ERR_BAD_ARG.  Each call writes one row of float64 accumulators
 * per sample into rows[B][K] (counts are float64 too: exact below 2^53).  Per-pixel quantities are the reference's float32 values
 * bit for bit (separately rounded products and sums, correctly rounded sqrt and division); only the accumulation is float64.
 * Two launches (one partial row per 2048 pixels into `workspace`, then a fixed-order fold per sample): no atomics, no counters,
 * every workspace slot of the launch's geometry is rewritten by each call, so rows are bitwise reproducible and do not depend on how
 * samples were batched.  workspace (8-byte aligned) >= the matching *_workspace_bytes query (0 for bad sizes).
 *   um_flow_metrics   over valid >= 0.5 (NULL: every pixel), epe = |pred - gt|, mag = |gt|:
 *                     0 n | 1 sum epe | 2..4 n of epe > 1, 3, 5 | 5 n of epe > 3 and epe / mag > 0.05 (KITTI outliers) |
 *                     6,7 n and sum epe of mag < 10 | 8,9 of 10 <= mag <= 40 | 10,11 of mag > 40 | with noc_valid (else zeros):
 *                     12,13 n and sum epe of matched pixels (noc_valid > 0.5 and the ground-truth target in frame:
 *                     0 <= x + u <= w - 1, 0 <= y + v <= h - 1, |u| <= w - 1, |v| <= h - 1) | 14,15 of the unmatched ones.
 *   um_disp_metrics   over gt > 0 (and gt < max_disp when max_disp > 0), e = |gt - pred|:
 *                     0 n | 1 sum e | 2..4 n of e > 1, 2, 3 | 5 n of e > 3 and e / gt > 0.05 (D1) |
 *                     6 n of e > 10 and e / max(gt, 1) > 0.1 (bad pixel) | 7 zero.
 *   um_depth_metrics  over lo < gt < hi and valid > 0.5 (NULL: no mask):
 *                     0 n | 1 sum |gt - pred| / gt | 2 sum (gt - pred)^2 / gt | 3 sum (gt - pred)^2 | 4 sum (ln gt - ln pred)^2,
 *                     float64 logarithms of the float32 values | 5..7 n of max(gt / pred, pred / gt) < 1.25, 1.25^2, 1.25^3. */
#define UM_FLOW_METRICS_K 16
#define UM_DISP_METRICS_K 8
#define UM_DEPTH_METRICS_K 8
size_t um_flow_metrics_workspace_bytes(int batch, int h, int w);
int um_flow_metrics(const float* pred, const float* gt, const float* valid, const float* noc_valid, double* rows, int batch, int hp,
                    int wp, int h, int w, int top, int left, void* workspace, size_t ws_bytes, void* stream);
size_t um_disp_metrics_workspace_bytes(int batch, int h, int w);
int um_disp_metrics(const float* pred, const float* gt, double* rows, int batch, int hp, int wp, int h, int w, int top, int left,
                    float max_disp, void* workspace, size_t ws_bytes, void* stream);
size_t um_depth_metrics_workspace_bytes(int batch, int h, int w);
int um_depth_metrics(const float* pred, const float* gt, const float* valid, double* rows, int batch, int hp, int wp, int h, int w,
                     int top, int left, float lo, float hi, void* workspace, size_t ws_bytes, void* stream);

/* Inference-size handling (csrc/prepost.hip): the block the reference's evaluation scripts repeat around the forward
 * (evaluate_flow.py:713-758, evaluate_stereo.py:340-375, evaluate_depth.py:78-129), as two memory-bound launches without state,
 * workspace or atomics.  "Image space" is the frame after the optional transpose: ih x iw = (transpose ? w x h : h x w).
 *   um_image_prepare  src: `batch` images of stored size h x w, UM_IMG_F32_NCHW [B,3,h,w] fp32 or UM_IMG_U8_NHWC [B,h,w,3] uint8 (a
 *                     decoder's frames) -> dst [B,3,hp,wp] fp32, in this order:
 *                       1. transpose != 0: H and W swap (the reference transposes tall inputs, evaluate_flow.py:713-717);
 *                       2. mean, std != NULL (HOST arrays of 3, as in um_conv7_fwd; both or neither, std != 0):
 *                          (x / 255 - mean) / std, three separately rounded fp32 operations (dataloader/stereo/transforms.py:20-63);
 *                          flow passes raw 0..255 values and NULL;
 *                       3. UM_SIZE_PAD: replicate padding with the image at (top, left): top + ih <= hp, left + iw <= wp (the
 *                          InputPadder geometry in both its modes), or UM_SIZE_RESIZE: bilinear, align_corners=True (top, left unused).
 *   um_pred_restore   the inverse, for a prediction pred [B,C,hp,wp] fp32 -> out [B,C,h,w] fp32 (C = 2 for UM_PRED_FLOW, 1 for
 *                     UM_PRED_DISPARITY / UM_PRED_DEPTH): UM_SIZE_PAD crops ih x iw at (top, left); UM_SIZE_RESIZE resizes to
 *                     ih x iw and rescales, a multiply and then a divide as the reference writes it: flow u * iw / wp and
 *                     v * ih / hp (evaluate_flow.py:754-755), disparity * iw / wp (evaluate_stereo.py:375), depth nothing
 *                     (evaluate_depth.py:131).  transpose != 0: the result is transposed back into h x w.  The flow CHANNELS ARE NOT
 *                     SWAPPED by that transpose: channel 0 is still the displacement along image-space x, exactly as the reference
 *                     leaves it (evaluate_flow.py:757-758).
 * Bilinear arithmetic is ATen's, in fp32: scale = float(in - 1) / float(out - 1) (0 when out == 1), src = scale * dst, i0 = (int)src,
 * i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1; the horizontal blends l0 a + l1 b of image space first, then the vertical one;
 * no fused multiply-add.  The reference's numbers come from F.interpolate, so this mirrors it rather than an exact rational
 * coordinate.  batch * C <= 65535 and every one of h, w, hp, wp <= UM_PREPOST_MAX_DIM (rows are spread over one grid dimension);
 * a bad argument returns UM_ERR_BAD_ARG. */
#define UM_PREPOST_MAX_DIM 262140
#define UM_IMG_F32_NCHW 0
#define UM_IMG_U8_NHWC 1
#define UM_SIZE_PAD 0
#define UM_SIZE_RESIZE 1
#define UM_PRED_FLOW 0
#define UM_PRED_DISPARITY 1
#define UM_PRED_DEPTH 2
int um_image_prepare(const void* src, int src_layout, float* dst, int batch, int h, int w, int transpose, const float* mean,
                     const float* std, int mode, int hp, int wp, int top, int left, void* stream);
int um_pred_restore(const float* pred, float* out, int batch, int channels, int hp, int wp, int mode, int top, int left, int h, int w,
                    int kind, int transpose, void* stream);
/* The same two launches with a horizontal mirror of image-space x as their LAST step, for the flipped views of the reference's
 * stereo inference (evaluate_stereo.py:790-841: resize, then hflip; resize back and rescale, then hflip):
 *   um_image_prepare_flip  hflip != 0: dst[..., x] = prepared[..., wp - 1 - x], `prepared` being what um_image_prepare writes.
 *   um_pred_restore_flip   hflip != 0: out[..., x] = restored[..., w - 1 - x], `restored` being what um_pred_restore writes.
 * The mirror is an index remap inside the one launch: the bilinear arithmetic is evaluated at the mirrored destination index, so the
 * result is torch.flip(<unflipped result>, [-1]) bit for bit (a resize of a mirrored source would differ in fp32).  hflip == 0 is
 * um_image_prepare / um_pred_restore, which delegate here. */
int um_image_prepare_flip(const void* src, int src_layout, float* dst, int batch, int h, int w, int transpose, const float* mean,
                          const float* std, int mode, int hp, int wp, int top, int left, int hflip, void* stream);
int um_pred_restore_flip(const float* pred, float* out, int batch, int channels, int hp, int wp, int mode, int top, int left, int h,
                         int w, int kind, int transpose, int hflip, void* stream);

/* Scalar map -> colour image (csrc/visualize.hip): the reference's vis_disparity and viz_depth_tensor (utils/visualization.py:11-16,
 * 92-107) per image of a batch.  x [B,h,w] fp32 -> rgb [B,h,w,3] uint8 = lut[idx], lut a DEVICE table [256][3]; stats_out (device,
 * may be NULL) receives [B][2] = vmin, vmax.  All arithmetic on values is fp32, every operation rounded on its own, IEEE division:
 *   v = inverse != 0 ? 1.0f / x : x;  vmin = the image's minimum of v.
 *   UM_NORM_MINMAX_255   vmax = the image's maximum; idx = (uint8) trunc(((v - vmin) / (vmax - vmin)) * 255.0f).
 *   UM_NORM_MIN_P95_256  vmax = the 95th percentile, linear: k = 0.95 (n - 1) in float64, lo = floor(k), hi = min(lo + 1, n - 1),
 *                        t = k - lo, vmax = (float)((double)a[lo] + ((double)a[hi] - (double)a[lo]) * t) with a the EXACT order
 *                        statistics of v (a radix select over order-preserving keys: a[lo], a[hi] are elements of the input whatever
 *                        the distribution); xa = ((v - vmin) / (vmax - vmin)) * 256.0f; idx = 255 if xa >= 256, else trunc(xa)
 *                        clamped to 0..255; idx = 0 for the whole image if vmax == vmin.
 * NaN or infinite values of v are outside the reference contract (NumPy's own result then depends on its version): the call
 * terminates, stays in bounds and gives a pixel whose normalised value is NaN index 0 (so a constant image under
 * UM_NORM_MINMAX_255 is all index 0); nothing more is promised for them.
 * Launches: per radix digit (11, 11, 10 bits) one histogram launch (LDS histograms, one partial per workgroup into `workspace`)
 * and one fold per image in index order, then the colour launch; UM_NORM_MINMAX_255 needs the first pair only, without a histogram.
 * No global atomics, no counters; every workspace slot that is read was written by the same call.  workspace (8-byte aligned) >=
 * um_scalar_to_rgb_workspace_bytes(batch, h, w) (0 for bad sizes); batch <= 65535, h * w <= 2^30. */
#define UM_NORM_MINMAX_255 0  /* vis_disparity */
#define UM_NORM_MIN_P95_256 1 /* viz_depth_tensor */
size_t um_scalar_to_rgb_workspace_bytes(int batch, int h, int w);
int um_scalar_to_rgb(const float* x, unsigned char* rgb, int batch, int h, int w, int inverse, int norm, const unsigned char* lut,
                     float* stats_out, void* workspace, size_t ws_bytes, void* stream);

/* The per-scale loop's small glue ops (round 3: they were torch calls):
 *   um_flow_upsample2x  out[B,V,2h,2w] = mult * bilinear_up2(flow[B,V,h,w]), align_corners = True -- unimatch/unimatch.py:162-163
 *                       (F.interpolate(..., scale_factor=2, mode='bilinear', align_corners=True) * 2: pass mult = 2)
 *   um_depth_cam_pack   cam[B or 2B][30] = Kinv | R | t | K (row major) from intrinsics [B,3,3] with rows 0-1 divided by stride_div
 *                       (unimatch.py:147-150) and pose [B,4,4]; with bidir, entries B..2B-1 carry the inverse pose
 *                       (matching.py:226-233).  Closed-form inverses (adjugate / determinant, evaluated in fp64, rounded once):
 *                       no torch.inverse (which synchronises the device).  A SINGULAR K or rotation cannot raise as
 *                       torch.inverse does: its inverse is all NaN, so that sample's predictions are NaN (other samples untouched).
 *                       Intrinsics / poses held in double by the caller are rounded to fp32 before the call.
 *   um_rigid_flow       flow[B,2,h,w] induced by inv_depth [B,1,h,w] and cam [B][30]: unimatch/geometry.py:99-195 as called
 *                       from the depth refinement (unimatch.py:295-305)
 *   um_relative_pose_pairs  rel[T-1,4,4]: rel[t] = inv(poses[t+1]) @ poses[t] from T >= 2 absolute camera-to-world poses [T,4,4]
 *                       (row major), the relative pose evaluate_depth.py:347-350 forms per pair on the host; the input of
 *                       um_depth_cam_pack for the consecutive pairs of a posed video.  A pose is taken as affine, [A t; 0 0 0 1]
 *                       (its bottom row is not read): inv = [A^-1, -A^-1 t] with the adjugate inverse of um_depth_cam_pack, the
 *                       product formed in fp64 and each of the 12 upper entries rounded to fp32 once; the bottom row is written
 *                       as exactly 0 0 0 1.  One thread per pair, no LU, no synchronisation.  A SINGULAR A in poses[t+1] makes
 *                       the upper three rows of rel[t] all NaN and touches no other pair.  A null pointer or frames < 2: -1. */
int um_flow_upsample2x(const float* flow, float* out, int batch, int channels, int h, int w, float mult, void* stream);
int um_depth_cam_pack(const float* intrinsics, const float* pose, float* cam, int batch, float stride_div, int bidir, void* stream);
int um_rigid_flow(const float* inv_depth, const float* cam, float* flow, int batch, int h, int w, void* stream);
int um_relative_pose_pairs(const float* poses, float* rel, int frames, void* stream);

/* Cross-view consistency and point clouds (csrc/geometry.hip): what a caller does with predicted disparities / depths of several
 * views.  Memory-bound, one thread per pixel; every entry point enqueues on `stream` and never synchronises; no global atomics, no
 * counters, nothing kept between calls; fp32 arithmetic with every product, sum, quotient and square root rounded on its own.
 * batch * h * w < 2^31.  A null pointer (where not stated as optional) or a bad size returns UM_ERR_BAD_ARG and names the entry point
 * in um_last_error_string.  Invalid values (NaN, inf, non-positive depths, a singular camera) never cause an out-of-bounds read: taps
 * are taken from clamped addresses and discarded.
 *   um_disp_consistency   the left / right check of a rectified pair: disp_left, disp_right [B,H,W] fp32 -> occ_left, occ_right
 *                         [B,H,W] fp32 in {0, 1}, 1 = occluded.  It is um_fwd_bwd_occlusion on the flows fwd = (-disp_left, 0) and
 *                         bwd = (+disp_right, 0), evaluated without the zero channel: the other view's disparity is sampled linearly
 *                         along the row at x - dL(x) (for the right view at x + dR(x)) -- two taps, zeros outside, the same
 *                         normalise / un-normalise round trip of the x coordinate -- and a pixel is occluded where
 *                         |dL - dR'| > alpha (|dL| + |dR|) + beta.  As in the flow check both magnitudes of the threshold are the
 *                         unwarped ones at the pixel itself; only the difference uses the sampled dR'.  W >= 2 (H >= 1).
 *   um_depth_consistency  the round trip of every pixel of a reference view through a source view: depth_ref, depth_src [B,H,W] fp32
 *                         METRIC depths (not inverse), cam_fwd, cam_inv [B][30] the Kinv | R | t | K records of um_depth_cam_pack at
 *                         stride_div = 1 for the ref -> src pose and for its inverse (the two halves of a bidir pack) -> occ [B,H,W]
 *                         fp32 in {0, 1} and, when not NULL, err_px, err_rel [B,H,W] fp32.  Per pixel p = (x, y) with d = depth_ref(p):
 *                           1. (u, v) = project(R (d Kinv p) + t) of cam_fwd, the divisor clamped at 1e-3 (unimatch/geometry.py:99-154);
 *                           2. in view iff 0 <= u <= W - 1 and 0 <= v <= H - 1;
 *                           3. s = bilinear sample of depth_src at (u, v): taps floor and min(floor + 1, size - 1), weights
 *                              (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay, summed in that order, taps of weight zero skipped;
 *                           4. X' = R' (s Kinv (u, v, 1)) + t' of cam_inv; d' = X'_z, p' = project(X') as in step 1;
 *                           5. err_px = |p' - p|, err_rel = |d' - d| / d;
 *                           6. occ = 0 iff err_px < px_thr and err_rel < rel_thr.
 *                         The pixel is occluded with both errors +inf when d is not finite or <= 0, when it is out of view, or when a
 *                         tap of non-zero weight is not finite or <= 0.  One launch, whatever the number of directed pairs in B.
 *   um_points_pack        a dense world-space point list of the selected pixels of depth [B,H,W] fp32: cam_world [B][30] is the cam
 *                         record of (intrinsics, camera-to-world pose); keep [B,H,W] fp32 (NULL: all; non-zero = keep); colors
 *                         [B,H,W,3] uint8 and rgb both NULL or both given.  Pixel (b, y, x) is selected iff x % stride == 0 and
 *                         y % stride == 0, it is kept, and its depth is finite with min_depth < d < max_depth.  The selected pixels
 *                         are written as xyz[n] = R (d Kinv p) + t (fp32 [N,3]) and rgb[n] = colors[b, y, x], n ascending in
 *                         (b, y, x): a STABLE compaction, n is the pixel's rank among the selected ones (what torch.nonzero gives).
 *                         count (one int32 ON THE DEVICE) receives N; xyz / rgb must hold a row for every candidate pixel
 *                         (B ceil(H / stride) ceil(W / stride)).  Three launches: one count per workgroup of 256 pixels (wave-64
 *                         ballot + popcount) into `workspace`, one workgroup's exclusive scan of the counts (which writes `count`),
 *                         and a scatter at scanned offset + rank inside the workgroup.  Every workspace slot that is read was written
 *                         by the same call; the order does not depend on scheduling.  workspace (4-byte aligned) >=
 *                         um_points_workspace_bytes(batch, h, w, stride) (0 for bad sizes), else UM_ERR_WORKSPACE. */
int um_disp_consistency(const float* disp_left, const float* disp_right, float* occ_left, float* occ_right, int batch, int h, int w,
                        float alpha, float beta, void* stream);
int um_depth_consistency(const float* depth_ref, const float* depth_src, const float* cam_fwd, const float* cam_inv, float* occ,
                         float* err_px, float* err_rel, int batch, int h, int w, float px_thr, float rel_thr, void* stream);
size_t um_points_workspace_bytes(int batch, int h, int w, int stride);
int um_points_pack(const float* depth, const float* cam_world, const float* keep, const unsigned char* colors, float* xyz,
                   unsigned char* rgb, int* count, int batch, int h, int w, int stride, float min_depth, float max_depth, void* workspace,
                   size_t ws_bytes, void* stream);

/* Volumetric fusion of posed depth maps (csrc/fusion.hip): a truncated signed distance (TSDF) volume averages the depths of all views,
 * weighted, and yields ONE surface at a size that does not grow with the video.  One thread per voxel; both entry points
 * enqueue on `stream`, never synchronise, use no atomics and keep nothing between calls; fp32 arithmetic with every product, sum and
 * quotient rounded on its own: each is bitwise equal to its host restatement (unimatch_amd/fusion.py).
 * Volume state (caller-owned, fp32, contiguous, x fastest): tsdf [nz,ny,nx] in units of the truncation distance, in [-1, 1]; weight
 * [nz,ny,nx] >= 0; color [3,nz,ny,nx] (optional planes, running means in 0..255).  A fresh volume is all zeros.  Voxel (i, j, k) has
 * the world centre X = (ox + (float)i voxel, oy + (float)j voxel, oz + (float)k voxel), origin = {ox, oy, oz} a HOST array read before
 * the call returns.  nx * ny * nz < 2^31.  A null pointer (where not stated as optional), a non-positive size, voxel / trunc /
 * max_weight not greater than 0 (or NaN), a colour pointer without its partner or an oversized volume returns UM_ERR_BAD_ARG and names
 * the entry point in um_last_error_string, before any device call.  No input value -- NaN, infinity, a singular camera -- causes an
 * out-of-bounds access: taps are read from clamped addresses and discarded.
 *   um_tsdf_integrate   depth [B,H,W] fp32 METRIC; cam_view [B][30] the WORLD-TO-CAMERA records: the second half of a bidirectional
 *                       um_depth_cam_pack of the intrinsics and the camera-to-world pose at stride_div = 1; weight_in [B,H,W] fp32 or
 *                       NULL (= 1); colors [B,H,W,3] uint8, NULL exactly when color is NULL.  B * H * W < 2^31.  ONE launch for all B
 *                       views: each voxel is owned by one thread that applies the views in ascending b with the running state in
 *                       registers, so the volume is read once and written once per call whatever B is, and one B-view call equals B
 *                       one-view calls bit for bit.  A voxel that no view updated is not written.  Per voxel (x, y, z) and view, with
 *                       c = cam_view[b]:
 *                          1. Xc_r = c[9+3r] x + c[10+3r] y + c[11+3r] z + c[18+r], summed left to right (r = 0, 1, 2);
 *                          2. zz = c[27] Xc_0 + c[28] Xc_1 + c[29] Xc_2; skip the view unless zz > 1e-3;
 *                          3. u = (c[21] Xc_0 + c[22] Xc_1 + c[23] Xc_2) / zz, v likewise with c[24..26];
 *                          4. px = rintf(u), py = rintf(v): the NEAREST pixel (interpolating depth across a discontinuity would
 *                             invent surfaces);
 *                          5. skip unless 0 <= px <= W - 1 and 0 <= py <= H - 1 (a NaN position skips);
 *                          6. d = depth[b, py, px]; skip unless d is finite and min_depth < d < max_depth;
 *                          7. w = weight_in ? weight_in[b, py, px] : 1; skip unless w is finite and w > 0;
 *                          8. sdf = d - Xc_2; skip unless sdf >= -trunc (so a NaN skips too);
 *                          9. f = fminf(1, sdf / trunc);
 *                         10. Wn = W + w, tsdf = (tsdf W + f w) / Wn;
 *                         11. each colour plane: C = (C W + (float)colors[b, py, px, ch] w) / Wn;
 *                         12. W = fminf(Wn, max_weight).
 *   um_tsdf_points      the surface points of the volume, in a deterministic order: candidates in ascending (k, j, i), then by axis
 *                       x, y, z.  The candidate of voxel p and axis a is the edge from p to its neighbour n = p + e_a where that
 *                       neighbour is inside the volume; it is a crossing iff weight(p) >= min_weight and weight(n) >= min_weight,
 *                       (tp < 0) != (tn < 0), and fabsf(tp) < 1 and fabsf(tn) < 1 (the last drops free-space-to-unseen jumps at
 *                       occlusion borders).  With s = tp / (tp - tn) its point is X(p) with coordinate a increased by s voxel, and its
 *                       colour rint(Cp + s (Cn - Cp)) clamped to 0..255.  xyz [capacity,3] fp32, rgb [capacity,3] uint8 (rgb given
 *                       exactly when color is).  A STABLE compaction built as um_points_pack is: per-workgroup counts (wave-64 ballot
 *                       + popcount) into `workspace`, one workgroup's exclusive scan, a scatter at scanned offset + rank; every
 *                       workspace slot that is read was written by the same call.  count (one int32 ON THE DEVICE) always receives
 *                       the full N (N < 2^31 is assumed); rows n >= capacity are not written: the caller runs again with a larger
 *                       buffer when N > capacity (capacity >= 0).  workspace (4-byte aligned) >=
 *                       um_tsdf_points_workspace_bytes(nx, ny, nz) (0 for bad sizes), else UM_ERR_WORKSPACE. */
int um_tsdf_integrate(const float* depth, const float* cam_view, const float* weight_in, const unsigned char* colors, float* tsdf,
                      float* weight, float* color, int nx, int ny, int nz, const float* origin, float voxel, float trunc,
                      float max_weight, float min_depth, float max_depth, int batch, int h, int w, void* stream);
size_t um_tsdf_points_workspace_bytes(int nx, int ny, int nz);
int um_tsdf_points(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const float* origin, float voxel,
                   float min_weight, float* xyz, unsigned char* rgb, int* count, int capacity, void* workspace, size_t ws_bytes,
                   void* stream);

/* The triangle mesh of a TSDF volume (csrc/tsdf_mesh.hip): marching tetrahedra on the Kuhn split of every cell -- six tetrahedra around
 * the main diagonal, the same split in every cell, so neighbouring cells agree on every face diagonal and the mesh is watertight by
 * construction; no case table, no ambiguous case.  Volume state, grid, argument rules and the bitwise agreement with the host
 * restatement (unimatch_amd/fusion.py: extract_mesh_host) are those of um_tsdf_points; the call enqueues on `stream`, never
 * synchronises, uses no atomics and keeps nothing.  A corner or edge mask m in 0..7 has bit 0 = +x, bit 1 = +y, bit 2 = +z; p + m adds
 * those unit steps to the voxel p = (i, j, k); t(p), w(p) are its stored value and weight.
 *   valid voxel    w(p) >= min_weight and fabsf(t(p)) < 1 (false for NaN): the rule of um_tsdf_points.
 *   active cell    cell c = (i, j, k) with i < nx - 1, j < ny - 1, k < nz - 1 whose eight corners c + m are all valid.
 *   inside         t < 0; a stored 0 counts as outside.
 *   edges          voxel p owns the seven edges (p, e), e = 1..7, from p to p + e: three axis edges (1, 2, 4), three face diagonals
 *                  (3, 5, 6), the body diagonal (7).  Edge (p, e) lies in the cells p - s for every subset s of the bits not in e
 *                  (those inside the grid), and carries a vertex when (t(p) < 0) != (t(p + e) < 0) and at least one of its cells is
 *                  active: no vertex is unreferenced.
 *   vertex         s = tp / (tp - tn) with tp = t(p), tn = t(p + e); coordinate a is base_a + s voxel where bit a is set in e, else
 *                  base_a, base = (ox + (float)i voxel, ...); colour rint(Cp + s (Cn - Cp)) clamped to 0..255, NaN -> 0.  For e in
 *                  {1, 2, 4} the vertex is bit for bit the point um_tsdf_points emits for that edge.
 *   vertex order   ascending (k, j, i, e).
 *   tetrahedra     tetrahedron tau = 0..5 of a cell belongs to the permutation pi of (0, 1, 2), in lexicographic order (0,1,2) (0,2,1)
 *                  (1,0,2) (1,2,0) (2,0,1) (2,1,0), of sign sigma = + - - + + -.  Its corners are the masks v0 = 0, v1 = 1 << pi0,
 *                  v2 = v1 | 1 << pi1, v3 = 7; the edge between vq and vr (q < r) is the owned edge (c + vq, vr ^ vq), its vertex
 *                  index E(q, r) = E(r, q).
 *   faces          per tetrahedron, I the inside positions ascending, O the outside positions ascending:
 *                    |I| = 0 or 4   no face;
 *                    |I| = 1, a = I[0]: the triangle (E(a,O0), E(a,O1), E(a,O2)), reversed iff (sigma > 0) == (a odd);
 *                    |I| = 3, a = O[0]: the triangle (E(a,I0), E(a,I1), E(a,I2)), reversed iff NOT ((sigma > 0) == (a odd));
 *                    |I| = 2, a < b inside, c < d outside: the quad q = (E(a,c), E(a,d), E(b,d), E(b,c)) as (q0,q1,q2) and (q0,q2,q3),
 *                                   both reversed iff (sigma > 0) == ((a + b) even);
 *                  reversed: (x, y, z) -> (z, y, x).  Every face is then counter-clockwise seen from free space (t > 0).
 *   face order     ascending (k, j, i) of the cell, then tau, then the triangle number; a face is three int32 indices into the FULL
 *                  vertex list.
 *   degenerate     a corner that stores exactly 0 gives s = 0 or 1 and triangles of zero area; they are kept (the topology stays
 *                  manifold).
 * xyz [vertex_capacity,3] fp32, rgb [vertex_capacity,3] uint8 (NULL exactly when color is NULL), faces [face_capacity,3] int32, counts
 * [2] int32 ON THE DEVICE: counts[0] = V and counts[1] = F always receive the full numbers (< 2^31 assumed).  Vertex rows >=
 * vertex_capacity and face rows >= face_capacity are not written; a face row that is written holds the true indices even where they
 * exceed vertex_capacity.  Both capacities >= 0.  workspace (4-byte aligned) >= um_tsdf_mesh_workspace_bytes(nx, ny, nz) (0 for bad
 * sizes; 7 bytes per voxel and 16 per 256 voxels), else UM_ERR_WORKSPACE; every workspace byte that is read was written by the same
 * call. */
size_t um_tsdf_mesh_workspace_bytes(int nx, int ny, int nz);
int um_tsdf_mesh(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const float* origin, float voxel,
                 float min_weight, float* xyz, unsigned char* rgb, int* faces, int* counts, int vertex_capacity, int face_capacity,
                 void* workspace, size_t ws_bytes, void* stream);

/* Frame synthesis from flow (csrc/interp.hip): apply a flow to the frames it was computed from.  A classical synthesis with no learned
 * part.  Memory-bound, one thread per pixel; every entry point enqueues on `stream` and never synchronises; nothing is kept between
 * calls.  fp32 arithmetic with every product, sum and quotient rounded on its own, float64 and int64 where stated; each entry point
 * is bitwise equal to its host restatement (unimatch_amd/interp.py).  Images are UM_IMG_F32_NCHW [B,C,H,W] fp32 or UM_IMG_U8_NHWC
 * [B,H,W,3] uint8; flows [B,2,H,W] fp32 (x, y); h, w >= 2; batch <= 65535.  A null pointer (where not stated as optional), a bad size
 * or a workspace that is too small returns UM_ERR_BAD_ARG and names the entry point in um_last_error_string.  NaN, infinite or huge
 * flows never cause an out-of-bounds access: taps are taken from clamped addresses and discarded.
 *   um_image_warp        out(p) = bilinear(image, p + flow(p)), the reference's flow_warp (unimatch/geometry.py:41-72) on an image:
 *                        out has the layout and type of image (uint8: rint of the fp32 sum, clamped to 0..255; channels == 3 there).
 *                        The position goes through the reference's normalise / un-normalise round trip (g = 2 p / (n - 1) - 1,
 *                        i = ((g + 1) / 2) (n - 1)), as in um_fwd_bwd_occlusion.  border == 0: taps outside the frame add nothing
 *                        (grid_sample's zeros padding); border != 0: the position is clamped into [0, w - 1] x [0, h - 1] first (a
 *                        NaN goes to 0).  mask (optional, [B,H,W] bytes in {0, 1}): the reference's return_mask, -1 <= g <= 1 in x
 *                        and y (before the clamp).  h * w <= 2^30.
 *   um_flow_splat        forward splatting of one or two flow fields (flow_bwd, weight_fwd, weight_bwd optional) to k <=
 *                        UM_INTERP_MAX_TIMES times each.  times: a HOST array [dirs][k] (dirs = 2 with flow_bwd, else 1), every
 *                        value strictly between 0 and 1; it is read before the call returns.  Source pixel p = (x, y) with flow
 *                        (u, v) lands at X = (float)x + t u, Y = (float)y + t v; ax = X - floor(X), ay likewise; its four taps
 *                        (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay are multiplied by weight[b, y, x] ([B,H,W] fp32, clamped
 *                        to <= 1; a weight that is NaN, infinite or <= 0 contributes nothing) and every in-frame tap adds, with
 *                        wq = (int64) rint(wt 65536), uq = (int64) rint(256 u), vq likewise:  S_w += wq, S_u += wq uq, S_v += wq vq.
 *                        A pixel whose flow is not finite or exceeds 32768 px in either component contributes nothing.  The sums are
 *                        64-bit INTEGER atomic adds: they commute, so the accumulators are bitwise reproducible from run to run
 *                        (float atomic sums depend on arrival order).  workspace (8-byte aligned) receives them as int64
 *                        [dirs][B][k][3][H][W] (planes S_w, S_u, S_v) and must hold um_flow_splat_workspace_bytes(batch, dirs, k,
 *                        h, w) bytes (0 for bad sizes).  The entry point clears the workspace itself on `stream` before the launch:
 *                        safe under graph capture, and no launch reads what an earlier call left behind.  |S| <= H W 2^39, so
 *                        H * W IS CAPPED AT 2^21 here (2^30 elsewhere would let the sums pass 2^63); batch * dirs * k <= 65535.
 *                        Optional outputs (a second launch when either is given): avg_out [dirs][B][k][2][H][W] fp32 =
 *                        (float)((double)S_u / (double)S_w / 256.0) (v likewise), and hole_out [dirs][B][k][H][W] bytes in {0, 1} =
 *                        S_w < max(1, rint(min_weight 65536)) (the product in fp32; 0 <= min_weight <= 1); avg_out is 0 in a hole.
 *   um_frame_synthesize  k in-between frames of every pair: out [B][k][H][W][3] uint8 and, optionally, holes [B][k][H][W] bytes.
 *                        img0, img1 in either layout (C = 3, values 0..255); accum: the accumulators of um_flow_splat for dirs = 2
 *                        with times = [t_0 .. t_k-1 | 1 - t_0 .. 1 - t_k-1] (the same HOST array is passed here); occ_fwd, occ_bwd
 *                        optional [B,H,W] fp32, 1 = occluded (um_fwd_bwd_occlusion).  Per output pixel q and time t, with
 *                        t' = times[1][.]:
 *                          1. A = the forward flow splatted to t, B = the backward flow splatted to t', each valid where its S_w
 *                             reaches the hole threshold; m = 0.5 (A + (-B)) when both are valid, A or -B when one is, else 0 and
 *                             q is a hole;
 *                          2. c0 = bilinear(img0, q - t m), c1 = bilinear(img1, q + t' m), positions clamped into the frame;
 *                             v0, v1 = the unclamped position lies in [0, w - 1] x [0, h - 1];
 *                          3. o0 = occ_fwd at q - t m, o1 = occ_bwd at q + t' m (bilinear, zeros outside; 0 without masks);
 *                          4. w0 = v0 ? t' (1 - o1) : 0, w1 = v1 ? t (1 - o0) : 0; if !(w0 + w1 >= 1e-6): w0 = t', w1 = t;
 *                          5. out = rint((w0 c0 + w1 c1) / (w0 + w1)) clamped to 0..255.
 *                        Bilinear taps NW, NE, SW, SE with the weights (x1 - x)(y1 - y) ... of um_fwd_bwd_occlusion, summed in
 *                        that order.  Same limits as um_flow_splat; accum_bytes >= um_flow_splat_workspace_bytes(batch, 2, k, h, w). */
#define UM_INTERP_MAX_TIMES 16
int um_image_warp(const void* image, int layout, const float* flow, void* out, unsigned char* mask, int batch, int channels, int h,
                  int w, int border, void* stream);
size_t um_flow_splat_workspace_bytes(int batch, int dirs, int k, int h, int w);
int um_flow_splat(const float* flow_fwd, const float* flow_bwd, const float* weight_fwd, const float* weight_bwd, const float* times,
                  int batch, int k, int h, int w, float min_weight, float* avg_out, unsigned char* hole_out, void* workspace,
                  size_t ws_bytes, void* stream);
int um_frame_synthesize(const void* img0, const void* img1, int layout, const float* occ_fwd, const float* occ_bwd, const float* times,
                        const void* accum, size_t accum_bytes, unsigned char* out, unsigned char* holes, int batch, int k, int h, int w,
                        float min_weight, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder helper (outside the hot path of SURVEY.md section 8; added because the element-wise tail of the CNN encoder
 * had become the largest non-convolution cost):  fused InstanceNorm2d(affine=False) + ReLU (+ shortcut + ReLU),
 *   t = (x - mean) * rsqrt(var + eps) per (image, channel) plane; relu != 0: t = max(t, 0);
 *   shortcut != NULL: t = max(t + shortcut, 0).
 * Replaces nn.InstanceNorm2d + nn.ReLU (+ residual add + ReLU) of unimatch/backbone.py:7-36.
 * x, shortcut, y: [planes, hw] fp32 contiguous (NCHW with planes = N*C, hw = H*W, hw % 4 == 0).
 * ------------------------------------------------------------------------------------------- */
int um_instance_norm_fwd(const float* x, const float* shortcut, float* y, long planes, int hw, float eps,
                         int relu, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: collecting the predictions (SURVEY.md 8b "allgather_preds", 8e).
 *
 * The path shards by sample (one process per GPU, contiguous batch split, weights replicated) and needs no collective
 * to COMPUTE; the one exchange is an all-gather of the final prediction over RCCL / xGMI.  The reference has no
 * inference-time collective; its process-group bring-up (utils/dist_utils.py:12-30, launcher
 * scripts/gmflow_scale1_train.sh:12) is what um_comm_* replaces, torch-free:
 *   um_comm_unique_id   rank 0 obtains the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means
 *                       (torch.distributed store, MPI, a file);
 *   um_comm_init_rank   every rank: ncclCommInitRank on the calling thread's current HIP device;
 *   um_comm_init_file   both steps through a file on a filesystem all ranks see: rank 0 publishes `path` atomically, the
 *                       others poll for it up to timeout_seconds (< 0: forever).  The caller chooses a job-unique path; rank 0
 *                       removes a leftover at `path` first, the record carries the world size and a wall-clock stamp (records
 *                       older than 10 minutes are ignored) and rank 0 deletes it once every rank has joined.
 *   um_comm_init_file_nonce  the same with a caller-chosen per-job nonce stored in the record: readers skip records of another
 *                       nonce, so a job relaunched under the same path right after a crash (leftover record still fresh) never
 *                       joins the dead id.  um_comm_init_file is nonce 0 on both sides.
 *   um_allgather_preds  ncclAllGather(send, recv, count_per_rank floats) enqueued on `stream` (the caller's compute or side
 *                       stream; no host synchronisation).  recv: [world][count_per_rank], rank major.
 *   um_comm_world       number of ranks of the communicator (ncclCommCount);  um_comm_destroy releases it.
 * RCCL is bound at first use by soname (librccl.so.1); without it these return UM_ERR_UNSUPPORTED.  The communicator is
 * the ONLY state the library ever holds on behalf of a caller, and it is an explicit handle.
 * ------------------------------------------------------------------------------------------- */
#define UM_COMM_ID_BYTES 128
int um_comm_unique_id(void* id_out /* UM_COMM_ID_BYTES, host */);
int um_comm_init_rank(void** comm_out, const void* id /* UM_COMM_ID_BYTES, host */, int rank, int world);
int um_comm_init_file(void** comm_out, const char* path, int rank, int world, int timeout_seconds);
int um_comm_init_file_nonce(void** comm_out, const char* path, int rank, int world, int timeout_seconds, int nonce);
int um_comm_world(void* comm);
int um_comm_destroy(void* comm);
int um_allgather_preds(void* comm, const float* send, float* recv, size_t count_per_rank, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SURVEY.md 8(b) names.  The survey's contract lists um_<op> / um_workspace_bytes_<op>; where this header spells an
 * entry point differently the literal name is exported too (csrc/aliases.hip, thin forwards):
 *   um_swin_attn_fwd          = um_window_attn_fwd                             (attention.py:8-16, 45-104)
 *   um_attn1d_fwd             = um_window_attn_fwd with win_h = 1, shift_h = 0 (attention.py:19-42, 107-163)
 *   um_local_corr_softmax_1d  = um_local_corr_softmax with one_d = 1           (matching.py:154-200)
 *   um_workspace_bytes_<op>(batch_or_streams, h, w, channels, mode)            (0 where um_<op> takes no workspace)
 * ------------------------------------------------------------------------------------------- */
int um_swin_attn_fwd(const float* q, const float* k, const float* v, float* out, int streams, int h, int w, int channels,
                     int win_h, int win_w, int shift_h, int shift_w, int mode, void* workspace, size_t workspace_bytes,
                     void* stream);
int um_attn1d_fwd(const float* q, const float* k, const float* v, float* out, int streams, int h, int w, int channels,
                  int win_w, int shift_w, int mode, void* workspace, size_t workspace_bytes, void* stream);
int um_local_corr_softmax_1d(const float* f0, const float* f1, float* out, int batch, int h, int w, int channels, int radius,
                             void* stream);
size_t um_workspace_bytes_swin_attn_fwd(int streams, int h, int w, int channels, int mode);
size_t um_workspace_bytes_attn1d_fwd(int streams, int h, int w, int channels, int mode);
size_t um_workspace_bytes_global_corr_softmax_flow(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_global_corr_softmax_stereo(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_prop_global_attn(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_local_corr_softmax(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_local_corr_softmax_1d(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_local_corr_with_flow(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_prop_local_attn(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_depth_corr_softmax(int batch, int h, int w, int channels, int mode);
size_t um_workspace_bytes_allgather_preds(int batch, int h, int w, int channels, int mode);

/* =============================================================================================
 * DIAGNOSTIC BUILDS ONLY (`python -m unimatch_amd.build --variant diag` -> unimatch_amd/_variants/libdiag.so, loaded through
 * UM_LIB): hardware micro-benchmarks behind -DUM_DIAGNOSTIC_BUILD (csrc/microbench.hip).  The shipped libunimatch_hip.so
 * exports NO um_debug_* symbol (tests/test_host_logic_cpu.py::test_library_exports_every_declared_symbol).
 * ============================================================================================= */
#ifdef UM_DIAGNOSTIC_BUILD
/* Diagnostic: a memory-free loop of independent 32x32x16 fp16 MFMAs on every CU (8 * iters MFMAs per wave, 1024 workgroups of
 * 8 waves): the sustained matrix-pipe rate of this part under its power limit, with one constant operand value or with
 * pseudo-random operands (data toggling costs clock).  sink: any device float. */
int um_debug_mfma_peak(float* sink, int iters, int random_operands, void* stream);
/* Diagnostic: the same loop with s_memtime stamps -- 256 workgroups of `waves` (4 | 8) waves, 8 * iters MFMAs per wave, on one accumulator
 * (`chain`) or four; ticks[256 * waves] receives every wave's elapsed s_memtime ticks.  With the host's wall time of the launch this
 * calibrates the tick rate and the ticks per MFMA the attention kernel's section stamps are read against (tools/mfma_ticks.py). */
int um_debug_mfma_ticks(unsigned long long* ticks, float* sink, int iters, int random_operands, int waves, int chain, void* stream);
/* Diagnostic: the attention kernel's QK^T pattern alone -- 256 workgroups of 4 waves, per "tile" 16 ds_read_b128 two k-steps ahead of the 24
 * MFMAs they feed (mode 0), or the same stream with the MFMAs on loop-invariant A registers (mode 1); ticks[1024]. */
int um_debug_mfma_lds(unsigned long long* ticks, float* sink, int tiles, int mode, void* stream);
#endif /* UM_DIAGNOSTIC_BUILD */

#ifdef __cplusplus
}
#endif
#endif /* UNIMATCH_HIP_H */
