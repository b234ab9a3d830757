"""Drop-in ``UniMatch`` module whose global-matching hot path runs on hand-written gfx950 HIP kernels.

Boundary (what a caller sees) is the reference's own:
``UniMatch(num_scales, feature_channels, upsample_factor, num_head, ffn_dim_expansion,
num_transformer_layers, reg_refine, task)`` (/root/reference/unimatch/unimatch.py:17-26),
``forward(img0, img1, attn_type, attn_splits_list, corr_radius_list, prop_radius_list, num_reg_refine,
pred_bidir_flow, task, intrinsics, pose, min_depth, max_depth, num_depth_candidates, depth_from_argmax,
pred_bidir_depth)`` -> ``{'flow_preds': [tensor]}`` (unimatch.py:95-111, 365-367) and the reference's
``state_dict`` names, so ``evaluate_flow/stereo/depth`` can drive it unchanged.

What is different inside:
  * features travel token-major ``[N, h*w, C]`` through the whole hot path (no permute/copy per window split);
  * self / cross attention is decided by the layer's role, not by a device->host sync on the data
    (reference: ``(query - key).abs().max() < 1e-6``, transformer.py:55);
  * attention, matching, propagation and the local cost volume are single fused HIP launches
    (``unimatch_amd.ops.HipOps``); no L x L, n x n or [B, L, C, taps] tensor is ever materialised;
  * inference only (the reference's training-mode extra outputs are out of scope).
  * the Transformer's linears / LayerNorm / FFN, the CNN encoder, the refinement block and the upsampler's mask head run
    on the same library (split-fp16 MFMA GEMM / implicit-GEMM convolution kernels, channels-last): on a GPU no MIOpen kernel
    or hipBLASLt kernel is left in the flow, stereo and depth forwards (rocprofv3 kernel statistics of all five configs: profiles/).
There is no CPU or PyTorch fallback for the hot path (the stock ``nn.Module`` convolution code only runs on CPU tensors).
"""
import math
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .encoder import CNNEncoder
from .refine import BasicUpdateBlock, convex_upsample
from .refine_nhwc import NhwcUpdateBlock
from .dist import shard_batch, shard_bounds
from .streams import PartRunner, forward_parts
from .confidence import depth_match_confidence, depth_match_multi_confidence, match_confidence

_IMAGENET_MEAN = (0.485, 0.456, 0.406)
_IMAGENET_STD = (0.229, 0.224, 0.225)


def attention_windows(attn_type, is_self, splits, h, w, with_shift):
    """(win_h, win_w, shift_h, shift_w) of one attention layer.

    Dispatch table of the reference (transformer.py:62-135) with the self/cross role made structural.
    2-D swin: K x K windows; 'row': every scanline; 'winrow': K windows per scanline; 'full': whole map.
    """
    if attn_type == 'swin':
        kind = 'win2d'
    elif attn_type == 'self_swin2d_cross_1d':
        kind = 'win2d' if is_self else 'row'
    elif attn_type == 'self_swin2d_cross_swin1d':
        kind = 'win2d' if is_self else 'winrow'
    else:
        kind = 'full'
    if splits <= 1:
        kind = {'win2d': 'full', 'winrow': 'row'}.get(kind, kind)
    if kind == 'full':
        return h, w, 0, 0
    if kind == 'row':
        return 1, w, 0, 0
    if kind == 'win2d':
        if h % splits or w % splits:
            raise AssertionError(f'feature map {h}x{w} is not divisible by attn_splits={splits}')
        wh, ww = h // splits, w // splits
        return (wh, ww, wh // 2, ww // 2) if with_shift else (wh, ww, 0, 0)
    if w % splits:
        raise AssertionError(f'feature width {w} is not divisible by attn_splits={splits}')
    ww = w // splits
    return (1, ww, 0, ww // 2) if with_shift else (1, ww, 0, 0)


def sine_position_tokens(win_h, win_w, reps_h, reps_w, channels):
    """Token-major ``[reps_h*win_h*reps_w*win_w, C]`` sine position table (fp32, CPU).

    Same arithmetic, in the same order, as the reference's DETR embedding evaluated on a window-sized grid
    (position.py:26-46, utils.py:114-124): normalised to 2*pi with eps 1e-6, temperature 10000, y features in
    the first C/2 channels.  The table is tiled over the reps_h x reps_w windows.
    """
    half = channels // 2
    ys = torch.arange(1, win_h + 1, dtype=torch.float32)
    xs = torch.arange(1, win_w + 1, dtype=torch.float32)
    ys = ys / (ys[-1] + 1e-6) * (2 * math.pi)
    xs = xs / (xs[-1] + 1e-6) * (2 * math.pi)
    j = torch.arange(half, dtype=torch.float32)
    dim_t = 10000.0 ** (2 * torch.div(j, 2, rounding_mode='floor') / half)

    def enc(v):
        ang = v[:, None] / dim_t
        out = torch.empty_like(ang)
        out[:, 0::2] = ang[:, 0::2].sin()
        out[:, 1::2] = ang[:, 1::2].cos()
        return out

    ey, ex = enc(ys), enc(xs)                                   # [win_h, half], [win_w, half]
    tab = torch.cat([ey[:, None, :].expand(win_h, win_w, half), ex[None, :, :].expand(win_h, win_w, half)], -1)
    return tab.repeat(reps_h, reps_w, 1).reshape(-1, channels).contiguous()


class TransformerLayer(nn.Module):
    """Attention (+ optional FFN) layer; parameters as in transformer.py:9-40, forward via HipOps."""

    def __init__(self, d_model, no_ffn, ffn_dim_expansion):
        super().__init__()
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.norm1 = nn.LayerNorm(d_model)
        self.no_ffn = no_ffn
        if not no_ffn:
            self.mlp = nn.Sequential(nn.Linear(2 * d_model, 2 * d_model * ffn_dim_expansion, bias=False), nn.GELU(),
                                     nn.Linear(2 * d_model * ffn_dim_expansion, d_model, bias=False))
            self.norm2 = nn.LayerNorm(d_model)

    def forward(self, ops, source, target, h, w, geom, kv_rotate=0, kv=None, next_kv_weights=None, fold=False, next_planes=False):
        """``kv_rotate = r`` (fused path only): ``target`` holds the streams in the SAME order as ``source`` and stream ``s``
        attends the keys / values of stream ``(s + r) mod S`` -- the swapped copy ``[f1; f0]`` is never built.
        ``kv = (k_operand, v_operand)``: the layer's key / value projections of ``target`` already exist as operand planes
        (``ops.kv4_slices``: the block projects both layers' k | v in one launch, or the previous block's FFN epilogue wrote them).
        ``fold``: ``kv`` holds the planes of ``target`` ITSELF, twice, and the attention runs with the folded weights ``Wk^T Wq`` /
        ``Wm Wv`` (``ops.fold_kv``); ``next_planes``: the FFN launch also returns the planes of its result, the next block's ``kv``."""
        if getattr(ops, 'fused_tail', False):
            return self._forward_fused(ops, source, target, h, w, geom, kv_rotate, kv, next_kv_weights, fold, next_planes)
        assert kv_rotate == 0 and kv is None and next_kv_weights is None and not fold and not next_planes
        q, k, v = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        msg = ops.window_attention(q, k, v, h, w, *geom)
        msg = self.norm1(self.merge(msg))
        if not self.no_ffn:
            msg = self.norm2(self.mlp(torch.cat([source, msg], dim=-1)))
        return source + msg

    def _forward_fused(self, ops, source, target, h, w, geom, kv_rotate=0, kv=None, next_kv_weights=None, fold=False, next_planes=False):
        """Same layer on the fused HIP path: projections emit attention operand planes, merge + LayerNorm
        (+ residual) is one kernel, the FFN is one kernel (``um_ffn_fwd``; or two without ``ops.fused_ffn``).
        ``next_kv_weights``: the four k | v projection weights of the NEXT block -- the FFN launch then also returns that
        block's blocked k | v planes (``ops.ffn_ln_kv``) and the result is ``(tokens, planes)``."""
        s, l, c = source.shape
        m = s * l
        src = source.reshape(m, c)
        if getattr(ops, 'fused_qproj', False) and getattr(ops, 'fused_merge', False):
            # q is projected inside the attention kernel's prologue (um_window_attn_qproj_merge_fwd): only k | v planes exist
            assert not fold or (kv is not None and next_kv_weights is None), 'the folded layer reads the planes of the stream itself'
            if kv is None:
                kvp, _, n2 = ops.linear_planes(target.reshape(m, c), (self.k_proj.weight, self.v_proj.weight))
                koff, voff = 0, c
                kop, vop = (kvp, m, n2, koff), (kvp, m, n2, voff)
            else:
                kop, vop = kv                                   # attention operands prepared by the block (ops.kv4_slices)
                assert kop[1] == m
            res = src if self.no_ffn else None
            if fold:                                            # keys = values = the tokens: k_proj / v_proj live in the folded weights
                msg = ops.window_attention_qproj_merge(src, self.q_proj.weight, kop, vop, s, h, w, *geom, kv_rotate, self.merge.weight,
                                                       self.norm1, res, fold=(self.k_proj.weight, self.v_proj.weight))
            else:
                msg = ops.window_attention_qproj_merge(src, self.q_proj.weight, kop, vop, s, h, w, *geom,
                                                       kv_rotate, self.merge.weight, self.norm1, res)
            if self.no_ffn:
                return msg
            msg = msg.reshape(m, c)
            if next_planes:
                out, npl = ops.ffn_ln(src, msg, self.mlp[0].weight, self.mlp[2].weight, self.norm2, planes=True)
                return out.reshape(s, l, c), npl
            if next_kv_weights is not None:
                out, nkv = ops.ffn_ln_kv(src, msg, self.mlp[0].weight, self.mlp[2].weight, self.norm2, next_kv_weights)
                return out.reshape(s, l, c), nkv
            if getattr(ops, 'fused_ffn', False):
                return ops.ffn_ln(src, msg, self.mlp[0].weight, self.mlp[2].weight, self.norm2).reshape(s, l, c)
            hid, _, nh = ops.linear_planes(src, (self.mlp[0].weight,), a1=msg, gelu=True)
            return ops.linear_ln(hid, (self.mlp[2].weight,), self.norm2, residual=src, a_planes_k=nh).reshape(s, l, c)
        assert kv is None and next_kv_weights is None and not fold and not next_planes, \
            'precomputed k | v planes need the fused q-projection / merge path'
        if target is source:                       # self attention: one projection launch for q | k | v
            qkv, _, n3 = ops.linear_planes(src, (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight))
            q, k, v = (qkv, m, n3, 0), (qkv, m, n3, c), (qkv, m, n3, 2 * c)
        else:
            qp, _, _ = ops.linear_planes(src, (self.q_proj.weight,))
            kv, _, n2 = ops.linear_planes(target.reshape(m, c), (self.k_proj.weight, self.v_proj.weight))
            q, k, v = (qp, m, c, 0), (kv, m, n2, 0), (kv, m, n2, c)
        if getattr(ops, 'fused_merge', False):      # merge + LayerNorm (+ residual) inside the attention kernel
            res = src if self.no_ffn else None
            msg = ops.window_attention_merge(q, k, v, s, h, w, *geom, kv_rotate, self.merge.weight, self.norm1, res)
            if self.no_ffn:
                return msg
            msg = msg.reshape(m, c)
        else:
            att = ops.window_attention_planes(q, k, v, s, h, w, *geom, kv_rotate=kv_rotate).reshape(m, c)
            if self.no_ffn:
                return ops.linear_ln(att, (self.merge.weight,), self.norm1, residual=src).reshape(s, l, c)
            msg = ops.linear_ln(att, (self.merge.weight,), self.norm1)
        if getattr(ops, 'fused_ffn', False):      # one kernel, the [M, 8C] hidden activations never reach HBM
            return ops.ffn_ln(src, msg, self.mlp[0].weight, self.mlp[2].weight, self.norm2).reshape(s, l, c)
        hid, _, nh = ops.linear_planes(src, (self.mlp[0].weight,), a1=msg, gelu=True)
        return ops.linear_ln(hid, (self.mlp[2].weight,), self.norm2, residual=src, a_planes_k=nh).reshape(s, l, c)


class TransformerBlock(nn.Module):
    def __init__(self, d_model, ffn_dim_expansion):
        super().__init__()
        self.self_attn = TransformerLayer(d_model, True, ffn_dim_expansion)
        self.cross_attn_ffn = TransformerLayer(d_model, False, ffn_dim_expansion)


class FeatureTransformer(nn.Module):
    """6 x (self-attention, cross-attention + FFN) on both images at once (transformer.py:203-294)."""

    def __init__(self, num_layers=6, d_model=128, nhead=1, ffn_dim_expansion=4):
        super().__init__()
        if nhead != 1:
            raise NotImplementedError('multi-head attention is not implemented (neither does the reference, '
                                      'transformer.py:63-66)')
        self.d_model = d_model
        self.layers = nn.ModuleList([TransformerBlock(d_model, ffn_dim_expansion) for _ in range(num_layers)])
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, ops, tok0, tok1, h, w, attn_type, attn_num_splits, stream=None):
        """tok0, tok1: ``[B, h*w, C]`` token-major features (position already added) -- or ``stream`` = the two already
        stacked as ``[2B, h*w, C]`` (what the encoder's batched output is: no concatenation copy)."""
        if stream is None:
            stream = torch.cat([tok0, tok1], 0)        # updated stream  [f0; f1]
        b = stream.shape[0] // 2
        rotate = getattr(ops, 'fused_tail', False)     # cross-attention target [f1; f0] = `prev` read with the halves rotated
        prev = stream if rotate else torch.cat([stream[b:], stream[:b]], 0)
        fused_attn = rotate and getattr(ops, 'fused_qproj', False) and getattr(ops, 'fused_merge', False)
        s2, l, c = stream.shape
        # both layers of a block read their keys / values from the stream AS IT ENTERS the block (self: the stream itself; cross:
        # its halves rotated).  ops.fold_kv: no k | v projection at all.  The layer is single-head and bias-free with nothing
        # non-linear between the projections and the attention (transformer.py:23-27, 58-60, 137), so k_proj / v_proj are folded into
        # the query and merge weights (ops.fold_weights) and keys = values = the stream: ONE planes tensor [NS][M][128] of the entering
        # stream serves both layers of the block -- block 0's by one format pass, every later one's written by the previous block's
        # FFN launch (um_ffn_planes_fwd).  block_kv / fused_kv then play no role.
        fold = fused_attn and getattr(ops, 'fold_kv', False)
        fold_ffn = fold and getattr(ops, 'fused_ffn', False)
        planes = None
        # without the fold the four projections Wk_self | Wv_self | Wk_cross | Wv_cross are ONE launch that reads the stream once and
        # writes blocked operand planes [NS][4][M][128] (um_kv4_fwd; round 4 -- was two um_linear_fwd launches of two projections
        # each: transformer.py:58-60 per layer)
        block_kv = fused_attn and not fold and getattr(ops, 'block_kv', True)
        # ... and from block 1 on they come out of the previous block's FFN launch (um_ffn_kv_fwd): no projection launch at all
        fused_kv = block_kv and getattr(ops, 'fused_kv', False) and getattr(ops, 'fused_ffn', False)
        kv4 = None
        kvw = lambda b_: (b_.self_attn.k_proj.weight, b_.self_attn.v_proj.weight, b_.cross_attn_ffn.k_proj.weight,
                          b_.cross_attn_ffn.v_proj.weight)
        for i, blk in enumerate(self.layers):
            shift = ('swin' in attn_type) and attn_num_splits > 1 and i % 2 == 1
            g_self = attention_windows(attn_type, True, attn_num_splits, h, w, shift)
            g_cross = attention_windows(attn_type, False, attn_num_splits, h, w, shift)
            kv_s = kv_c = None
            if fold:
                if planes is None:                     # block 0 (or the two-launch FFN): the stand-alone format pass
                    planes, _, _ = ops.linear_planes(stream.reshape(s2 * l, c), ())
                kv_s = kv_c = ((planes, s2 * l, c, 0),) * 2
                planes = None
            if block_kv:
                if kv4 is None:                        # block 0 (or fused_kv off): the stand-alone launch
                    kv4 = ops.kv4_planes(stream.reshape(s2 * l, c), kvw(blk))
                kv_s, kv_c = ops.kv4_slices(kv4, s2 * l)
                kv4 = None
            stream = blk.self_attn(ops, stream, stream, h, w, g_self, kv=kv_s, fold=fold)
            if rotate:                                 # keys / values come from the stream as it was before this block
                nxt = kvw(self.layers[i + 1]) if fused_kv and i + 1 < len(self.layers) else None
                nxp = fold_ffn and i + 1 < len(self.layers)
                stream = blk.cross_attn_ffn(ops, stream, prev, h, w, g_cross, kv_rotate=b, kv=kv_c, next_kv_weights=nxt, fold=fold,
                                            next_planes=nxp)
                if nxt is not None:
                    stream, kv4 = stream
                elif nxp:
                    stream, planes = stream
                prev = stream
            else:
                stream = blk.cross_attn_ffn(ops, stream, prev, h, w, g_cross)
                prev = torch.cat([stream[b:], stream[:b]], 0)
        return stream[:b].contiguous(), stream[b:].contiguous()


class SelfAttnPropagation(nn.Module):
    """Flow propagation with feature self-similarity (attention.py:166-253); parameters only."""

    def __init__(self, in_channels):
        super().__init__()
        self.q_proj = nn.Linear(in_channels, in_channels)
        self.k_proj = nn.Linear(in_channels, in_channels)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, ops, tok0, flow, h, w, local_window_attn=False, local_window_radius=1):
        if hasattr(ops, 'linear_bias') and tok0.is_cuda:              # the library's own biased Linear (um_linear_bias_fwd)
            if not local_window_attn:
                # reference quirk kept on purpose: the global path projects the *query* again (attention.py:198-205)
                return ops.prop_global_projected(tok0, self.q_proj, self.k_proj, flow, h, w)
            b, l, c = tok0.shape
            x = tok0.reshape(b * l, c)
            q = ops.linear_bias(x, self.q_proj.weight, self.q_proj.bias).view(b, l, c)
            k = ops.linear_bias(x, self.k_proj.weight, self.k_proj.bias).view(b, l, c)
            return ops.prop_local(q, k, flow, h, w, local_window_radius)
        q = self.q_proj(tok0)                                         # injected CPU oracle backend (host-logic tests)
        if local_window_attn:
            return ops.prop_local(q, self.k_proj(tok0), flow, h, w, local_window_radius)
        return ops.prop_global(q, self.k_proj(q), flow, h, w)


def _to_tokens(fmap):
    return fmap.flatten(2).transpose(1, 2).contiguous()


def _to_map(tokens, h, w):
    b, _, c = tokens.shape
    return tokens.transpose(1, 2).reshape(b, c, h, w)


def _pixel_grid(h, w, device):
    ys, xs = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32),
                            torch.arange(w, device=device, dtype=torch.float32), indexing='ij')
    return torch.stack([xs, ys], 0)


def _warp(fmap, flow):
    """Bilinear warp with zero padding, align_corners (geometry.py:41-72); torch op, not on the hot path."""
    b, c, h, w = fmap.shape
    pos = _pixel_grid(h, w, fmap.device)[None] + flow
    grid = torch.stack([2 * pos[:, 0] / (w - 1) - 1, 2 * pos[:, 1] / (h - 1) - 1], -1)
    return F.grid_sample(fmap, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def _rigid_flow(depth, intrinsics, pose):
    """Flow induced by depth and relative pose (geometry.py:99-195)."""
    b, h, w = depth.shape
    grid = _pixel_grid(h, w, depth.device)
    homog = torch.cat([grid, torch.ones(1, h, w, device=depth.device)], 0).flatten(1)
    pts = (torch.inverse(intrinsics) @ homog) * depth.view(b, 1, -1)
    pts = pose[:, :3, :3] @ pts + pose[:, :3, 3:]
    proj = intrinsics @ pts
    return (proj[:, :2] / proj[:, 2:].clamp(min=1e-3)).view(b, 2, h, w) - grid


def neighbour_rows(nb, carried):
    """The row table ``[2, nb, 3]`` int32 (f0 row | f1 row | cam row) of a fused sequence chunk of ``nb`` consecutive pairs
    (``um_depth_corr_softmax_multi_rows``).  Token rows index the segments ``tok0 [nb] | tok1 [nb] | the carried pair's tok0, tok1 [2]``;
    cam rows index the bidirectional pack of ``n = nb + carried`` pairs, the carried pair first: forward cams ``[0, n)``, inverse cams
    ``[n, 2n)``.  Source 0 "next" of frame t is ``(t, nb + t, carried + t)``; source 1 "previous" is pair t - 1 seen from its second
    frame, ``(nb + t - 1, t - 1, n + carried + t - 1)`` -- the row that is f1 of one sample is f0 of the next.  Frame 0 takes the carried
    pair ``(2 nb + 1, 2 nb, n)`` or, without one, is off (-1: the launch never reads an off source)."""
    c = 1 if carried else 0
    n = nb + c
    t = torch.arange(nb, dtype=torch.int32)
    nxt = torch.stack([t, nb + t, c + t], 1)
    prv = torch.stack([nb + t - 1, t - 1, n + c + t - 1], 1)
    prv[0] = torch.tensor([2 * nb + 1, 2 * nb, n] if c else [-1, -1, -1], dtype=torch.int32)
    return torch.stack([nxt, prv], 0).contiguous()


class UniMatch(nn.Module):
    def __init__(self, num_scales=1, feature_channels=128, upsample_factor=8, num_head=1, ffn_dim_expansion=4,
                 num_transformer_layers=6, reg_refine=False, task='flow'):
        super().__init__()
        if feature_channels != 128:
            raise NotImplementedError('the HIP kernels are built for feature_channels=128 '
                                      '(the value of every released UniMatch model)')
        self.feature_channels = feature_channels
        self.num_scales = num_scales
        self.upsample_factor = upsample_factor
        self.reg_refine = reg_refine
        self.backbone = CNNEncoder(output_dim=feature_channels, num_output_scales=num_scales)
        self.transformer = FeatureTransformer(num_layers=num_transformer_layers, d_model=feature_channels,
                                              nhead=num_head, ffn_dim_expansion=ffn_dim_expansion)
        self.feature_flow_attn = SelfAttnPropagation(in_channels=feature_channels)
        if not reg_refine or task == 'depth':
            self.upsampler = nn.Sequential(nn.Conv2d(2 + feature_channels, 256, 3, 1, 1), nn.ReLU(inplace=True),
                                           nn.Conv2d(256, upsample_factor ** 2 * 9, 1, 1, 0))
        if reg_refine:
            self.refine_proj = nn.Conv2d(128, 256, 1)
            self.refine = BasicUpdateBlock(corr_channels=(2 * 4 + 1) ** 2, downsample_factor=upsample_factor,
                                           flow_dim=2 if task == 'flow' else 1, bilinear_up=task == 'depth')
        # not part of the state_dict: hot-path backend and caches
        self._ops = None
        self._precision = 'exact'
        self._pos_cache = {}
        self.debug_taps = None            # set to a dict to collect named intermediates (diagnostics only)
        self.check_weights = False        # True: fingerprint the parameters every forward (see _check_weight_print)
        self._weight_print = None
        self._slots = None                # the submodules' parameter dicts (see _parameter_slots)
        self._runner = PartRunner()       # the batch as concurrent forwards (see forward)

    # ------------------------------------------------------------------ hot-path backend
    def set_precision(self, precision):
        """'exact' (fp16 hi+lo split MFMA operands; parity mode) or 'fast' (bf16 operands)."""
        self._precision = precision
        self._ops = None
        return self

    def invalidate_weights(self):
        """Drop the cached MFMA operand planes of the weights.  Needed only after an in-place edit through ``.data``
        (``p.data.mul_(2)`` changes neither the tensor's identity, version nor address); ``load_state_dict``, ``.to()`` /
        ``.float()`` / ``.cuda()`` and ``p.data = new`` are detected without it."""
        if self._ops is not None:
            self._ops.invalidate_weights()
        self._weight_print = None
        return self

    def _apply(self, fn, *args, **kwargs):            # .to() / .cuda() / .float(): parameters move, caches must not survive
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_weights()
        self._pos_cache = {}
        self._slots = None
        return out

    def _parameter_slots(self):
        """The ``_parameters`` dicts of all submodules, collected once (``self.parameters()`` walks the module tree and builds every
        name: some hundred microseconds, too much for a per-forward check).  The dicts are the modules' own: a parameter that is
        assigned anew shows up here; ``.to()`` and friends collect them again."""
        if self._slots is None:
            self._slots = [m._parameters for m in self.modules() if m._parameters]
        return self._slots

    def weights_state(self):
        """Identity, storage address, version and dtype of every parameter: what :meth:`HipOps._cache_get` keys a weight's planes by.
        Equal states (together with an unchanged ``HipOps.cache_generation``) mean that the planes a captured graph reads are still
        the planes of the current weights (``unimatch_amd.graph``)."""
        return tuple((id(p), p.data_ptr(), p._version, p.dtype) for d in self._parameter_slots() for p in d.values() if p is not None)

    def check_parameter_dtypes(self):
        """The kernels read biases and LayerNorm parameters in place, as fp32, through their address: a parameter of another dtype
        (``model.half()``) would be read past its end.  Weights are converted when their planes are built, but a model that is half
        converted is refused as a whole, before any launch."""
        for d in self._parameter_slots():
            for name, p in d.items():
                if p is not None and p.dtype is not torch.float32:
                    raise ValueError(f'the HIP forward reads parameters as float32, found {name} {tuple(p.shape)} of dtype {p.dtype}: '
                                     'convert the model with .float() (reduced precision is set_precision("fast"))')

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_weights()
        return out

    def _check_weight_print(self):
        """check_weights=True: a per-forward fingerprint of all parameters (one fused norm, one host sync) that catches
        in-place ``.data`` edits automatically -- off by default because the sync serialises back-to-back forwards.  The first
        fingerprint has nothing to be compared with: the planes that forwards before it cached (``check_weights`` switched on after
        an edit) are dropped once."""
        params = [p.detach() for p in self.parameters()]
        fp = torch.stack(torch._foreach_norm(params)).double().cpu()
        if self._weight_print is None or not torch.equal(fp, self._weight_print):
            if self._ops is not None:
                self._ops.invalidate_weights()
        self._weight_print = fp

    def bind_ops(self, ops):
        """Install a hot-path backend explicitly (tests inject the CPU oracle here)."""
        self._ops = ops
        return self

    @property
    def ops(self):
        if self._ops is None:
            from .ops import HipOps           # raises when the HIP extension or the GPU is missing
            self._ops = HipOps(self._precision)
        return self._ops

    def _position(self, h, w, splits, device):
        # same precondition as the reference's split_feature (unimatch/utils.py:40)
        assert splits <= 1 or (h % splits == 0 and w % splits == 0), \
            f'feature map {h}x{w} is not divisible by attn_splits={splits}'
        key = (h, w, splits, str(device))
        if key not in self._pos_cache:
            if splits > 1:
                tab = sine_position_tokens(h // splits, w // splits, splits, splits, self.feature_channels)
            else:
                tab = sine_position_tokens(h, w, 1, 1, self.feature_channels)
            self._pos_cache[key] = tab.to(device)
        return self._pos_cache[key]

    def _constants(self, device):
        """ImageNet mean / std on ``device``, uploaded once (keeps the forward free of host->device copies so that
        it can be captured into a HIP graph)."""
        key = ('imagenet', str(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = (torch.tensor(_IMAGENET_MEAN).view(1, 3, 1, 1).to(device),
                                    torch.tensor(_IMAGENET_STD).view(1, 3, 1, 1).to(device))
        return self._pos_cache[key]

    def _depth_candidates(self, lo, hi, n, device):
        """Inverse-depth candidates: computed on the CPU exactly as the reference does (unimatch.py:187), cached."""
        key = ('cand', float(lo), float(hi), int(n), str(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = torch.linspace(lo, hi, n).float().to(device).contiguous()
        return self._pos_cache[key]

    def _convex(self, flow2, mask, is_depth=False):
        ops = self.ops
        if hasattr(ops, 'convex_upsample') and flow2.is_cuda and self.upsample_factor in (4, 8):
            return ops.convex_upsample(flow2, mask, self.upsample_factor, is_depth)
        return convex_upsample(flow2, mask, self.upsample_factor, is_depth=is_depth)

    check_range = True       # read the operand-range flags at the start of every exact-mode forward (no synchronisation)

    def check_operand_range(self, sync=True):
        """Raise ``_abi.OperandRangeError`` if any exact-mode kernel met an activation outside fp16's range since the last check
        (``sync``: wait for the device first, so that the forward that has just been enqueued is covered)."""
        from . import _abi
        if sync and torch.cuda.is_available():
            torch.cuda.synchronize()
        _abi.check_operand_range()

    def _upsample_mask(self, flow2, f0_map):
        """The upsampler head (unimatch.py:56-58): convex-combination logits of the full-resolution prediction ->
        ``(mask, mask_is_nhwc)``; on the GPU the two convolutions run channels-last on the library's kernels."""
        ops = self.ops
        if getattr(ops, 'fused_conv', False) and flow2.is_cuda and self.upsample_factor in (4, 8):
            # cat(flow, feature) -> 3x3 + ReLU -> 1x1 -> NHWC mask
            b, v, h, w = flow2.shape
            rows = b * h * w
            feat = f0_map.permute(0, 2, 3, 1).reshape(rows, -1)          # a view when f0_map came from tokens
            c1, c2 = self.upsampler[0], self.upsampler[2]
            if getattr(ops, 'fused_glue', False) and v <= 4:
                # one launch builds the input planes; the hidden map leaves the 3x3's epilogue as the 1x1's operand planes
                planes, cin = ops.nhwc_concat_planes(flow2.contiguous(), feat.contiguous())
                hid = ops.cached_planes_buffer('upsampler_hidden', rows, c1.out_channels, flow2.device)
                ops.conv_ex((planes, cin, 0, cin), (b, h, w), (ops.conv_weight_planes(ops.conv_weight_padded(c1.weight, cin)), c1.bias),
                            (3, 3), 1, (1, 1), 1, outp=(hid, c1.out_channels, 0))
                mask, _, _ = ops.conv2d_nhwc((hid, b, h, w, c1.out_channels), c2.weight, c2.bias, 1, (0, 0))
                return mask, True
            planes, cin = ops.nhwc_planes_from([flow2.permute(0, 2, 3, 1).reshape(rows, v), feat])
            hid, _, _ = ops.conv2d_nhwc((planes, b, h, w, cin), ops.conv_weight_padded(c1.weight, cin), c1.bias, 1, (1, 1),
                                        relu=True)
            hp, hc = ops.nhwc_planes_from([hid])
            mask, _, _ = ops.conv2d_nhwc((hp, b, h, w, hc), c2.weight, c2.bias, 1, (0, 0))
            return mask, True
        return self.upsampler(torch.cat([flow2, f0_map], 1)), False

    def _upsample(self, flow2, f0_map, is_depth=False, out=None):
        """``out``: where the channels-last path writes the prediction (``HipOps.convex_upsample``); other paths ignore it."""
        mask, nhwc = self._upsample_mask(flow2, f0_map)
        if nhwc:
            return self.ops.convex_upsample(flow2, mask, self.upsample_factor, is_depth, mask_nhwc=True, out=out)
        return self._convex(flow2, mask, is_depth=is_depth)

    # ------------------------------------------------------------------ forward
    launch_parts = None      # None: streams.forward_parts() decides per call; an int forces that many concurrent forwards (1: never split)

    def forward(self, img0, img1, attn_type=None, attn_splits_list=None, corr_radius_list=None,
                prop_radius_list=None, num_reg_refine=1, pred_bidir_flow=False, task='flow', intrinsics=None,
                pose=None, min_depth=1. / 0.5, max_depth=1. / 10, num_depth_candidates=64,
                depth_from_argmax=False, pred_bidir_depth=False, **kwargs):
        """The reference's entry point (unimatch/unimatch.py:95-111), the only one a caller such as evaluate_flow.py:405-412 knows.

        Round 6: HOW the batch is launched is decided here, by a pure function of the call (``streams.forward_parts``): either one
        forward of the whole batch, or -- where the launches of one forward leave tails that a second forward fills (measured per
        configuration) -- the batch as two forwards of contiguous sample ranges on two HIP streams, joined on the caller's
        stream.  The samples of a batch are independent (unimatch.py:113-367 has no cross-sample operation), every part is bitwise
        the plain forward of its samples."""
        return self._forward_batch(img0, img1, self.launch_parts, attn_type, attn_splits_list, corr_radius_list, prop_radius_list,
                                   num_reg_refine, pred_bidir_flow, task, intrinsics, pose, min_depth, max_depth, num_depth_candidates,
                                   depth_from_argmax, pred_bidir_depth)

    def forward_with_confidence(self, img0, img1, **forward_kw):
        """:meth:`forward` plus ``'match_confidence'``: how sure the global matching step (``corr_radius == -1``) is of every
        feature pixel's match, from the same tokens the flow is matched on (``unimatch_amd.confidence``: statistics of the reference's
        ``prob``, which is never formed).  A dict of ``max_prob``, ``entropy``, ``variance`` ``[B', h, w]`` float, ``best``
        ``[B', h, w]`` int32 (token index; stereo: column), ``scale`` (the map's stride in image pixels) and, with
        ``pred_bidir_flow=True`` (``B' = 2B``: forward, then backward), ``mutual`` ``[B, h, w]`` bool.  Tasks ``'flow'`` and
        ``'stereo'``.  The batch runs as one forward; ``flow_preds`` is what :meth:`forward` returns with ``launch_parts = 1``."""
        task = forward_kw.get('task', 'flow')
        if task == 'depth':
            raise NotImplementedError("forward_with_confidence: task='depth' matches by a plane sweep over depth candidates, which has "
                                      "its own distribution; only 'flow' and 'stereo' have the global matching step "
                                      "(forward_with_depth_confidence returns the statistics of the plane sweep's distribution)")
        if -1 not in (forward_kw.get('corr_radius_list') or ()):
            raise ValueError('forward_with_confidence needs a global matching step (a corr_radius of -1 in corr_radius_list)')
        if forward_kw.get('pred_bidir_flow') and task != 'flow':
            raise ValueError(f"pred_bidir_flow is a flow option, got task={task!r}")
        conf = {}
        out = dict(self._forward_batch(img0, img1, 1, confidence=conf, **forward_kw))
        out['match_confidence'] = conf
        return out

    def forward_with_depth_confidence(self, img0, img1, *, peak_radius=1, **forward_kw):
        """:meth:`forward` for ``task='depth'`` plus ``'depth_confidence'``: statistics of the plane sweep's distribution over the
        inverse-depth candidates of every feature pixel (the reference's ``match_prob``, unimatch/matching.py:227, which is never
        formed).  A dict of ``max_prob``, ``entropy``, ``variance`` (about the soft-argmin, inverse depth squared), ``peak_mass`` (the
        probability within ``peak_radius`` candidates of the best one) ``[B', h, w]`` float, ``best`` (first arg-max candidate) and
        ``in_view`` (candidates that land inside the second view; 0: a uniform distribution) ``[B', h, w]`` int32, ``scale`` (the
        map's stride in image pixels) and ``num_candidates``; ``B' = 2B`` with ``pred_bidir_depth`` (forward, then backward).  The
        batch runs as one forward.  On the GPU the matching step is ONE launch (``um_depth_corr_softmax_stats``) that writes the
        prediction and the statistics; on host tensors the prediction comes from the backend as in :meth:`forward` and the statistics
        from ``confidence.depth_match_stats_host``."""
        task = forward_kw.get('task', 'flow')
        if task != 'depth':
            raise ValueError(f"forward_with_depth_confidence: the plane sweep is the matching step of task='depth', got task={task!r} "
                             "(forward_with_confidence serves 'flow' and 'stereo')")
        if isinstance(peak_radius, bool) or not isinstance(peak_radius, int) or peak_radius < 0:
            raise ValueError(f'peak_radius: expected an int >= 0, got {peak_radius!r}')
        conf = {}
        out = dict(self._forward_batch(img0, img1, 1, confidence=conf, peak_radius=peak_radius, **forward_kw))
        out['depth_confidence'] = conf
        return out

    def _sweep_multiview(self, ops, tok0, tok1, h, w, cam, cand, sources, use, from_argmax, scale, confidence, peak_radius):
        """The fused plane sweep of ``sources`` views per reference frame (tokens and ``cam`` source-major, ``[sources * B, ...]``):
        ``[B, 1, h, w]``.  CUDA tensors: one ``um_depth_corr_softmax_multi`` launch, which also writes the statistics when a
        ``confidence`` dict asks for them.  Host tensors: ``confidence.depth_match_logits_multi_host``.  One view that is on everywhere
        is the two-view sweep exactly as :meth:`forward` launches it (the fused launch at S = 1 always reduces the statistics and
        costs 1.09 x the plain one, profiles/depth_multiview.txt)."""
        b = tok0.shape[0] // sources
        f0, f1 = (t.contiguous().view(sources, b, h * w, t.shape[-1]) for t in (tok0, tok1))
        cams = cam.view(sources, b, 30)
        if confidence is not None:
            if sources == 1 and use is None:              # one view, on everywhere: the two-view sweep, as forward launches it
                out, conf = depth_match_confidence(ops, tok0, tok1, h, w, cam, cand, from_argmax, scale, peak_radius)
            else:
                out, conf = depth_match_multi_confidence(ops if tok0.is_cuda else None, f0, f1, h, w, cams, cand, use, from_argmax, scale,
                                                         peak_radius)
            confidence.update(conf)
            return out
        if sources == 1 and use is None:
            return ops.depth_corr_softmax(tok0, tok1, h, w, cam, cand, from_argmax)
        if tok0.is_cuda:
            return ops.depth_corr_softmax(f0, f1, h, w, cams, cand, from_argmax, use=use)
        from .confidence import depth_match_multi
        return depth_match_multi(f0, f1, h, w, cams, cand, use, from_argmax=from_argmax)[0]

    def _neighbour_rows(self, nb, carried, device):
        """:func:`neighbour_rows` on ``device``: a pure function of (pairs in the chunk, carry present), uploaded once per device and
        cached as ``_position`` and ``_constants`` are, so a warm call copies nothing and never waits for the device."""
        key = ('nbr_rows', int(nb), bool(carried), str(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = neighbour_rows(int(nb), bool(carried)).to(device)
        return self._pos_cache[key]

    def _sweep_neighbours(self, ops, tok0, tok1, h, w, intrinsics, pose, up, cand, neighbour, from_argmax, confidence, peak_radius):
        """The fused plane sweep of the ``nb`` consecutive pairs of a sequence chunk (``_match``'s ``neighbour``): ``(out [nb, 1, h, w],
        cam [nb, 30] of the forward pairs)``.  ONE cam pack of the carried pair and the chunk's pairs in both directions, ONE
        ``um_depth_corr_softmax_multi_rows`` launch on ``tok0``, ``tok1`` as the Transformer left them and the carried pair's two rows;
        host tensors go through ``confidence.depth_match_multi``'s restatement.  Leaves the last pair in ``neighbour['out']``."""
        from .confidence import depth_match_multi
        nb = tok0.shape[0]
        carried = neighbour['carry']
        c = 0 if carried is None else 1
        k_all, p_all = intrinsics, pose
        if c:
            k_all, p_all = torch.cat([carried['intrinsics'], intrinsics], 0), torch.cat([carried['pose'], pose], 0)
        if hasattr(ops, 'depth_cam') and tok0.is_cuda:
            cam_all = ops.depth_cam(k_all, p_all, float(up), True)
        else:
            kc = k_all.clone()
            kc[:, :2] = kc[:, :2] / up
            kc = kc.repeat(2, 1, 1)
            pc = torch.cat([p_all, torch.inverse(p_all)], 0)
            cam_all = torch.cat([torch.inverse(kc).flatten(1), pc[:, :3, :3].flatten(1), pc[:, :3, 3], kc.flatten(1)], 1).float().contiguous()
        rows = self._neighbour_rows(nb, c, tok0.device)
        tok0, tok1 = tok0.contiguous(), tok1.contiguous()              # they are: slices of the Transformer's output along dim 0
        segments = [tok0, tok1] + ([carried['tokens']] if c else [])
        if confidence is not None:
            out, conf = depth_match_multi_confidence(ops if tok0.is_cuda else None, segments, None, h, w, cam_all, cand, None, from_argmax,
                                                     up, peak_radius, rows=rows)
            confidence.update(conf)
        elif tok0.is_cuda:
            out = ops.depth_corr_softmax(segments, None, h, w, cam_all, cand, from_argmax, rows=rows)
        else:
            out = depth_match_multi(segments, None, h, w, cam_all, cand, from_argmax=from_argmax, rows=rows)[0]
        neighbour['out'] = {'tokens': torch.stack([tok0[nb - 1], tok1[nb - 1]], 0), 'pose': pose[nb - 1:].clone(),
                            'intrinsics': intrinsics[nb - 1:].clone()}
        return out, cam_all[c:c + nb]

    def forward_multiview(self, img_ref, img_srcs, *, intrinsics, poses, attn_type=None, attn_splits_list=None, prop_radius_list=None,
                          num_reg_refine=1, min_depth=1. / 0.5, max_depth=1. / 10, num_depth_candidates=64, depth_from_argmax=False,
                          pred_bidir_depth=False, task='depth', return_confidence=False, peak_radius=1):
        """Depth of ``img_ref [B, 3, H, W]`` from ``S`` source views ``img_srcs [B, S, 3, H, W]`` that vote in ONE plane sweep:
        ``{'flow_preds': [depth [B, H, W]]}``.  ``intrinsics [B, 3, 3]``, ``poses [B, S, 4, 4]`` = the relative pose reference ->
        source ``s`` in :meth:`forward`'s convention; the other keywords are :meth:`forward`'s for ``task='depth'``.

        Each of the ``B (1 + S)`` images is encoded once, the Transformer runs on the ``B S`` pairs as one stream (source-major), and
        the per-source logits are averaged over the sources that see a candidate before the one softmax (``um_depth_corr_softmax_multi``,
        csrc/depth_multi.hip).  Propagation, upsampling and refinement run on the primary pair ``s = 0`` exactly as in :meth:`forward`.
        This is an UNLEARNED extension: the weights are trained on two views; the mean over the seeing sources keeps the logits at the
        scale the softmax was trained at.  With ``S = 1`` the result is that of ``forward(img_ref, img_srcs[:, 0], task='depth', ...)``
        run as one part.  ``return_confidence=True`` adds ``'depth_confidence'``, the statistics of the FUSED distribution (the keys of
        :meth:`forward_with_depth_confidence`), from the sweep's own launch.  Depth only, one scale; ``pred_bidir_depth`` is refused (its backward prediction has no second source)."""
        if task != 'depth':
            raise ValueError(f"forward_multiview: the plane sweep is the matching step of task='depth', got task={task!r}")
        if self.num_scales != 1:
            raise ValueError('forward_multiview needs a one-scale model (num_scales == 1), as task=\'depth\' does')
        if pred_bidir_depth:
            raise ValueError('forward_multiview: pred_bidir_depth is a two-view option (the backward prediction has no second source)')
        if img_srcs.dim() != 5 or img_srcs.shape[0] != img_ref.shape[0] or tuple(img_srcs.shape[2:]) != tuple(img_ref.shape[1:]):
            raise ValueError(f'img_srcs: expected [B, S, 3, H, W] matching img_ref {tuple(img_ref.shape)}, got {tuple(img_srcs.shape)}')
        b, sources = img_srcs.shape[:2]
        if not 1 <= sources <= 8:
            raise ValueError(f'forward_multiview: 1 .. 8 source views, got {sources}')
        if tuple(poses.shape) != (b, sources, 4, 4) or tuple(intrinsics.shape) != (b, 3, 3):
            raise ValueError(f'expected intrinsics [{b}, 3, 3] and poses [{b}, {sources}, 4, 4], got {tuple(intrinsics.shape)} and {tuple(poses.shape)}')
        if isinstance(peak_radius, bool) or not isinstance(peak_radius, int) or peak_radius < 0:
            raise ValueError(f'peak_radius: expected an int >= 0, got {peak_radius!r}')
        if len(attn_splits_list or ()) != 1 or len(prop_radius_list or ()) != 1:
            raise ValueError('forward_multiview: attn_splits_list and prop_radius_list need one entry (one scale)')
        ops = self.ops
        if img_ref.is_cuda:
            self.check_parameter_dtypes()
        if self.check_weights:
            self._check_weight_print()
        dev = img_ref.device
        if img_ref.is_cuda and self.check_range and getattr(ops, 'mode', 1) == 0:
            from . import _abi
            _abi.check_operand_range('an earlier forward of this process: ')
        import contextlib
        guard = torch.cuda.device(dev) if img_ref.is_cuda else contextlib.nullcontext()
        conf = {} if return_confidence else None
        with guard, torch.no_grad():
            kw = dict(attn_type=attn_type if attn_type is not None else '', attn_splits_list=attn_splits_list,
                      prop_radius_list=prop_radius_list, num_reg_refine=num_reg_refine, task='depth', min_depth=min_depth,
                      max_depth=max_depth, num_depth_candidates=num_depth_candidates, depth_from_argmax=depth_from_argmax,
                      confidence=conf, peak_radius=peak_radius, sources=sources)
            if sources == 1:                              # the two-view call: the encoder and the stream of _forward_one
                img1 = img_srcs[:, 0].contiguous()
                with_pos = (not self.reg_refine and self.debug_taps is None and getattr(ops, 'fused_glue', False)
                            and self.backbone.takes_raw_images(ops, img_ref) and img_ref.shape == img1.shape)
                pos = (lambda h, w: self._position(h, w, attn_splits_list[0], dev)) if with_pos else None
                feats = self._encode((img_ref, img1), 'depth', pos)
                out = self._match(feats, b, stream_has_pos=with_pos, intrinsics=intrinsics, pose=poses[:, 0].contiguous(), **kw)
            else:
                # every image once: [ref; src_0; ...; src_{S-1}], then the stream of the B S pairs, source-major: [ref x S; sources]
                feats = self._encode((torch.cat([img_ref, img_srcs.transpose(0, 1).reshape((sources * b,) + tuple(img_ref.shape[1:]))], 0),), 'depth')
                feats = [torch.cat([f[:b].repeat(sources, 1, 1, 1), f[b:]], 0) for f in feats]
                out = self._match(feats, sources * b, intrinsics=intrinsics.repeat(sources, 1, 1),
                                  pose=poses.transpose(0, 1).reshape(sources * b, 4, 4).contiguous(), **kw)
        out = dict(out)
        if return_confidence:
            out['depth_confidence'] = conf
        return out

    _PREDICT_DEFAULTS = {'flow': (8, 'sintel', 'flow'), 'stereo': (32, 'sintel', 'disparity'), 'depth': (16, 'kitti', 'depth')}

    def predict(self, img0, img1, *, inference_size=None, padding_factor=None, pad_mode=None, transpose='auto', normalize=None,
                pred_right_disp=False, pred_bidir_disp=False, **forward_kw):
        """:meth:`forward` at an inference size, with the prediction back at the images' size: the block the reference's scripts
        repeat around the model (evaluate_flow.py:713-758, evaluate_stereo.py:340-375, evaluate_depth.py:78-129) through
        :class:`unimatch_amd.prepost.InferenceGeometry`.  Returns the forward's dict with ``flow_preds[-1]`` restored.

        ``img0``, ``img1``: fp32 ``[B, 3, H, W]`` or uint8 ``[B, H, W, 3]`` (a decoder's frames).  ``inference_size=(hp, wp)``
        resizes (bilinear, align_corners; flow and disparity are rescaled on the way back, depth is not); ``None`` pads to multiples
        of ``padding_factor`` as ``InputPadder(mode=pad_mode)`` does -- per task 8 / 'sintel' (flow), 32 / 'sintel' (stereo), 16 /
        'kitti' (depth) unless given.  ``transpose='auto'`` transposes tall flow inputs and nothing else (a stereo pair or a posed
        pair has no transposed meaning); the flow channels are not swapped back, as in the reference.  ``normalize``: ``None``
        means ``task != 'flow'`` for uint8 input (the ImageNet constants) and ``False`` for fp32 input, which the stereo and depth
        loaders have normalised already; flow is always normalised inside the model.  ``forward_kw`` goes to :meth:`forward`.
        On the GPU this adds three launches to the forward and never waits for the device.

        Stereo views (``task='stereo'`` only, else ``ValueError``; evaluate_stereo.py:790-841; consumed here, not passed on):
        ``pred_right_disp`` runs the model on ``(hflip(right), hflip(left))`` and mirrors the restored disparity back: the right
        view's disparity.  ``pred_bidir_disp`` runs ONE forward of batch 2B on ``[left; hflip(right)]``, ``[right; hflip(left)]`` and
        returns ``flow_preds[-1]`` ``[2B, H, W]``: the left view's disparities, then the right view's, mirrored back (the reference
        leaves that last mirror to its caller).  Both together follow the reference literally -- the doubling first, then the swap
        -- so the halves come out in the other order.  The mirrors are part of the prepare / restore launches (four prepares into
        the halves of two preallocated tensors, two restores into the halves of one): no ``torch.flip``, no ``torch.cat``."""
        from .prepost import InferenceGeometry, geometry_for, image_size
        task = forward_kw.get('task', 'flow')
        if task not in self._PREDICT_DEFAULTS:
            raise ValueError(f'task must be one of {sorted(self._PREDICT_DEFAULTS)}, got {task!r}')
        factor, mode, kind = self._PREDICT_DEFAULTS[task]
        if img0.is_cuda:
            self.check_parameter_dtypes()                 # before the prepare launches, not only before the forward's
        shape = image_size(img0)
        if image_size(img1) != shape or img1.dtype != img0.dtype:
            raise ValueError(f'img0 {tuple(img0.shape)} {img0.dtype} and img1 {tuple(img1.shape)} {img1.dtype} differ')
        if isinstance(transpose, str):
            transpose = InferenceGeometry._resolve_transpose(shape, transpose) and task == 'flow'
        geom = geometry_for(shape, inference_size, padding_factor or factor, pad_mode or mode, transpose)
        if normalize is None:
            normalize = img0.dtype == torch.uint8 and task != 'flow'
        if pred_right_disp or pred_bidir_disp:
            if task != 'stereo':
                raise ValueError(f"pred_right_disp / pred_bidir_disp are stereo views: task='stereo', got {task!r}")
            return self._predict_stereo_views(img0, img1, geom, normalize, bool(pred_right_disp), bool(pred_bidir_disp), forward_kw)
        a0, a1 = geom.prepare(img0, img1, normalize=normalize)
        out = dict(self(a0, a1, **forward_kw))
        preds = list(out['flow_preds'])
        preds[-1] = geom.restore(preds[-1], kind)
        out['flow_preds'] = preds
        return out

    def _predict_stereo_views(self, left, right, geom, normalize, right_disp, bidir, forward_kw):
        """The flipped / doubled stereo views of :meth:`predict`.  With L, R the prepared views and ' the mirror, the model sees
        right only ``(R', L')``; bidir only ``([L; R'], [R; L'])``; both ``([R'; L], [L'; R])`` (the doubled pair, swapped and
        mirrored).  On the way back a half is mirrored iff the model's first image of that half was a mirrored view."""
        if not bidir:
            a0, = geom.prepare(right, normalize=normalize, hflip=True)
            a1, = geom.prepare(left, normalize=normalize, hflip=True)
            out = dict(self(a0, a1, **forward_kw))
            preds = list(out['flow_preds'])
            preds[-1] = geom.restore(preds[-1], 'disparity', hflip=True)
            out['flow_preds'] = preds
            return out
        b = left.shape[0]
        a0 = torch.empty((2 * b, 3) + geom.size, dtype=torch.float32, device=left.device)
        a1 = torch.empty_like(a0)
        plain, mirrored = (slice(b, None), slice(0, b)) if right_disp else (slice(0, b), slice(b, None))
        geom.prepare(left, normalize=normalize, out=a0[plain])
        geom.prepare(right, normalize=normalize, out=a1[plain])
        geom.prepare(right, normalize=normalize, hflip=True, out=a0[mirrored])
        geom.prepare(left, normalize=normalize, hflip=True, out=a1[mirrored])
        out = dict(self(a0, a1, **forward_kw))
        preds = list(out['flow_preds'])
        pred = preds[-1]
        back = torch.empty((2 * b,) + geom.shape, dtype=torch.float32, device=pred.device)
        geom.restore(pred[plain], 'disparity', out=back[plain])
        geom.restore(pred[mirrored], 'disparity', hflip=True, out=back[mirrored])
        preds[-1] = back
        out['flow_preds'] = preds
        return out

    def _check_bidir_flow(self, pred_bidir_flow):
        """``pred_bidir_flow`` with refinement needs two scales: the reference stacks [forward; backward] features only at scale
        1 (unimatch.py:139-141), so on one scale its refinement meets B feature samples and 2B flows and fails in a ``view``.
        Raised here, before the encoder or the backend is touched."""
        if pred_bidir_flow and self.reg_refine and self.num_scales == 1:
            raise ValueError('pred_bidir_flow=True with reg_refine=True needs num_scales=2: at num_scales=1 the features are never '
                             'stacked [forward; backward] for the refinement (the reference fails there too)')

    def _forward_batch(self, img0, img1, parts, attn_type=None, attn_splits_list=None, corr_radius_list=None,
                       prop_radius_list=None, num_reg_refine=1, pred_bidir_flow=False, task='flow', intrinsics=None,
                       pose=None, min_depth=1. / 0.5, max_depth=1. / 10, num_depth_candidates=64,
                       depth_from_argmax=False, pred_bidir_depth=False, confidence=None, peak_radius=1, **kwargs):
        """:meth:`forward` with ``parts`` in place of ``launch_parts`` (``ConcurrentUniMatch`` forces its own count here).
        ``confidence``: a dict the matching step fills (:meth:`forward_with_confidence`, :meth:`forward_with_depth_confidence` with
        its ``peak_radius``; one part only)."""
        if self.training:
            raise RuntimeError('this module implements inference only: call .eval() '
                               '(training-mode auxiliary outputs of the reference are out of scope)')
        self._check_bidir_flow(pred_bidir_flow)
        kw = dict(attn_type=attn_type, attn_splits_list=attn_splits_list, corr_radius_list=corr_radius_list,
                  prop_radius_list=prop_radius_list, num_reg_refine=num_reg_refine, pred_bidir_flow=pred_bidir_flow, task=task,
                  intrinsics=intrinsics, pose=pose, min_depth=min_depth, max_depth=max_depth,
                  num_depth_candidates=num_depth_candidates, depth_from_argmax=depth_from_argmax, pred_bidir_depth=pred_bidir_depth)
        batch = img0.shape[0]
        parts = self._plan_parts(parts, task, attn_type, batch, img0.shape[-2], img0.shape[-1], img0.is_cuda)
        if parts <= 1:
            return self._forward_one(img0, img1, confidence=confidence, peak_radius=peak_radius, **kw)
        assert confidence is None, 'the matching confidence is collected by one forward of the whole batch'

        def prepare(r):
            pk = dict(kw, intrinsics=shard_batch(intrinsics, r, parts), pose=shard_batch(pose, r, parts))
            return shard_batch(img0, r, parts), shard_batch(img1, r, parts), pk

        def compute(r, ins, out=None):
            a0, a1, pk = ins
            return self._forward_one(a0, a1, pred_out=out, **pk)['flow_preds']

        bidir = 2 if (pred_bidir_flow or pred_bidir_depth) else 1
        # a flow prediction is written by the parts' last launches straight into one tensor: no concatenation at the join
        out_shape = None
        if task == 'flow' and bidir == 1 and img0.is_cuda and getattr(self.ops, 'fused_glue', False):
            out_shape = (batch, 2) + tuple(img0.shape[-2:])
        return self._runner.run_parts(self, parts, batch, bidir, img0.shape, img0.device, kw, prepare, compute, out_shape=out_shape)

    def _plan_parts(self, parts, task, attn_type, batch, height, width, is_cuda):
        """How many concurrent parts a call of ``batch`` samples runs as: ``parts`` when given (``launch_parts``), else
        ``streams.forward_parts`` (one with ``debug_taps``: the taps are per forward), never more than the batch."""
        if parts is None:
            parts = 1
            if is_cuda and self.debug_taps is None:
                parts = forward_parts(task, attn_type, self.num_scales, self.reg_refine, batch, height, width)
        return min(int(parts), batch)

    # ------------------------------------------------------------------ video: consecutive frames
    def _carry_state(self, frames):
        """What a carry is valid for: the model and backend objects (weak references), device, geometry, the backend's cache
        generation and the parameters' identity / versions."""
        ops = self._ops
        params = tuple((id(p), p.data_ptr(), p._version) for p in self.parameters())
        return ((weakref.ref(self), None if ops is None else weakref.ref(ops)),
                (str(frames.device), tuple(frames.shape[1:]), getattr(ops, 'cache_generation', None), params))

    def _carry_valid(self, carry, frames):
        refs, key = carry['state']
        now_refs, now_key = self._carry_state(frames)
        return (refs[0]() is self and (refs[1] is None) == (now_refs[1] is None) and (refs[1] is None or refs[1]() is self._ops)
                and key == now_key)

    def forward_sequence(self, frames, attn_type=None, attn_splits_list=None, corr_radius_list=None, prop_radius_list=None,
                         num_reg_refine=1, pred_bidir_flow=False, consistency_check=False, colorize=False, pairs_per_launch=8,
                         carry=None, task='flow', intrinsics=None, poses=None, min_depth=1. / 0.5, max_depth=1. / 10,
                         num_depth_candidates=64, depth_from_argmax=False, pred_bidir_depth=False, track_points=None,
                         return_confidence=False, interpolate=0, peak_radius=1, fuse_neighbours=False):
        """Optical flow of every pair (t, t+1) of a frame sequence ``frames [T, 3, H, W]`` (raw 0..255), each frame encoded ONCE.

        The reference's ``inference_flow`` (evaluate_flow.py:640-831) runs the model on each pair, so every interior frame goes through
        the CNN encoder twice.  The encoder is strictly per image, so here a chunk of ``pairs_per_launch`` pairs encodes only the frames
        not encoded yet (``B + 1`` images for ``B`` pairs, ``B`` with the previous chunk's last frame) and the match step runs on the
        stream ``[F[0:B]; F[1:B+1]]`` built by one concatenation per scale.  ``carry`` (the previous call's ``out['carry']``) continues a
        long video fed in pieces: its frame pairs with ``frames[0]``.  A carry made under another model, backend, device, geometry,
        backend cache generation or parameter version is not trusted: its stored frame is encoded again.

        Returns ``{'flow': [P, 2, H, W], 'carry': ...}`` with ``P = T - 1`` (``T`` with a carry), plus ``'flow_bwd'`` with
        ``pred_bidir_flow``, ``'occ_fwd'`` / ``'occ_bwd'`` ``[P, H, W]`` float with ``consistency_check`` (the reference's
        forward_backward_consistency_check) and ``'flow_rgb'`` (``'flow_bwd_rgb'``) ``[P, H, W, 3]`` uint8 with ``colorize`` (its
        flow_to_image, each image normalised by its own maximum).

        ``track_points`` (flow only) follows points of the call's first frame through the sequence (:func:`video.chain_flows`, one
        launch per chunk right after the chunk's flows): ``'dense'`` (every pixel), an int stride (every stride-th pixel of every
        stride-th row) or an ``[N, 2]`` tensor of (x, y).  The result gains ``'tracks' [P, N, 2]`` (positions in frame t + 1) and
        ``'tracks_visible' [P, N]`` bool; with ``pred_bidir_flow`` a track also ends where the chunk's forward occlusion mask covers
        it (the mask ``consistency_check`` returns, computed once), otherwise only where it leaves the frame.  The carry gains
        ``'track'`` (the last positions and flags); a later call with that carry and any ``track_points`` other than ``None``
        continues the same tracks (a tensor of another N raises).  ``None``: no tracking, and no ``'track'`` in the carry.

        ``return_confidence`` (flow only): the result gains ``'match_confidence'``, what :meth:`forward_with_confidence` returns, taken
        in the same forward at the chunk's global matching step: ``max_prob``, ``entropy``, ``variance``, ``best`` ``[P, h, w]`` of
        the forward direction, ``scale`` and, with ``pred_bidir_flow``, ``mutual`` ``[P, h, w]``.  A chunk then runs as one part.

        ``interpolate`` K >= 1 (flow only, needs ``pred_bidir_flow``): the result gains ``'frames_between'`` ``[P, K, H, W, 3]`` uint8,
        the K frames at the times ``k / (K + 1)`` between the two frames of every pair (:func:`interp.interpolate_frames`: a classical
        synthesis by flow splatting, backward warps and an occlusion-aware blend, with no learned part).  It is computed per chunk
        right after the chunk's flows (two launches), from the chunk's own frames and its occlusion masks (those of
        ``consistency_check`` / tracking, computed once).  0: nothing is launched and every other output is unchanged.

        ``task='depth'``: the depth of every frame t of a posed video from the pair (t, t + 1) -- the one other task whose consecutive
        pairs share a frame (a stereo pair shares nothing with the next one: ``task='stereo'`` raises).  ``frames`` are what
        :meth:`forward` takes for depth (normalised already), ``poses [T, 4, 4]`` the frames' absolute camera-to-world matrices and
        ``intrinsics`` ``[1, 3, 3]`` (one camera) or ``[T, 3, 3]`` (pair t uses row t for both views, as the reference does with the
        first image's).  The relative poses ``inv(poses[t + 1]) @ poses[t]`` of the whole call come from one launch
        (``HipOps.relative_pose_pairs``; fp32 ``torch.linalg.inv`` for CPU tensors) and each chunk's rows go into the match step
        of :meth:`forward` unchanged; ``min_depth`` ... ``pred_bidir_depth`` mean what they mean there.  The carry also holds the last
        frame's pose and intrinsics row.  Returns ``{'depth': [P, H, W], 'carry': ...}``, plus ``'depth_bwd'`` (the depth of frame t + 1
        seen from pair t) with ``pred_bidir_depth`` and ``'depth_rgb'`` (``'depth_bwd_rgb'``) ``[P, H, W, 3]`` uint8 with ``colorize``
        (``visualize.inverse_depth_to_image``).  With ``return_confidence`` the result gains ``'depth_confidence'``, what
        :meth:`forward_with_depth_confidence` returns (window ``peak_radius``), taken in the chunk's own plane-sweep launch: the maps
        ``[P, h, w]`` of the forward direction, ``scale`` and ``num_candidates``; a chunk then runs as one part.  On the GPU a depth call never waits for the device.  The depth keywords are ignored
        for ``task='flow'``.

        ``fuse_neighbours=True`` (depth only): the PREVIOUS frame votes in every frame's plane sweep as a second source view, for the
        price of the sweep alone.  The Transformer is symmetric in its two halves, so pair t - 1 has already produced frame t's tokens
        conditioned on frame t - 1 and frame t - 1's conditioned on frame t; with the inverse of that pair's relative pose (and that
        pair's intrinsics row, as ``pred_bidir_depth`` uses it) they are a second source of reference frame t.  Frame t >= 1 fuses source
        0 "next" ``(tok0[t], tok1[t], cam of pair t)`` and source 1 "previous" ``(tok1[t-1], tok0[t-1], inverse cam of pair t-1)`` in ONE
        launch per chunk (``um_depth_corr_softmax_multi_rows``: the operands are rows of the Transformer's output, named by a cached
        row table and not copied; the cam pack stays one launch per chunk); the logits are averaged over the sources that see a
        candidate before the one softmax, as in :meth:`forward_multiview`, which computes the same thing per frame at twice the
        Transformer work.  This is an UNLEARNED extension: the weights are trained on two views; the mean over the seeing sources
        keeps the logits at the scale the softmax was trained at.  Propagation, upsampling and refinement run on source 0 exactly as
        without the flag.  The keys and shapes of the result are unchanged (``'depth' [P, H, W]`` is the depth of frame t of pair t;
        the last frame of a video keeps having no entry); with ``return_confidence`` the statistics are those of the FUSED
        distribution, from the same launch.  A chunk runs as one part.  The carry gains ``'neighbour'``: the last pair's two token
        rows after the Transformer (cloned), its relative pose and its intrinsics row, which the next chunk -- of this call or of
        the next -- passes as a third segment, so a video fed in pieces that give the same chunk shapes gives the same bytes as one
        call.  The first frame of a call without a usable carry has source 1 OFF (the two-view distribution); so has the first frame
        after a stale carry (see above: its frame is encoded again) and after a carry made without the flag, which holds no
        ``'neighbour'``.  Refused with ``task='flow'`` and with ``pred_bidir_depth`` (the backward prediction is what the fused sweep
        replaces)."""
        if self.training:
            raise RuntimeError('this module implements inference only: call .eval()')
        if task == 'stereo':
            raise NotImplementedError("forward_sequence: consecutive stereo pairs share no frame, so there is nothing to encode once; "
                                      "batch the pairs through forward() / predict()")
        if task not in ('flow', 'depth'):
            raise ValueError(f"task must be 'flow' or 'depth', got {task!r}")
        if task == 'depth' and track_points is not None:
            raise ValueError("track_points follows points through optical flow: it needs task='flow'")
        if isinstance(peak_radius, bool) or not isinstance(peak_radius, int) or peak_radius < 0:
            raise ValueError(f'peak_radius: expected an int >= 0, got {peak_radius!r}')
        if isinstance(interpolate, bool) or not isinstance(interpolate, int) or not 0 <= interpolate <= 16:
            raise ValueError(f'interpolate: expected an int in 0 .. 16 (in-between frames per pair), got {interpolate!r}')
        if interpolate and task == 'depth':
            raise ValueError("interpolate synthesises frames from optical flow: it needs task='flow'")
        if interpolate and not pred_bidir_flow:
            raise ValueError('interpolate needs pred_bidir_flow=True (the flows of both directions)')
        if return_confidence and task == 'flow' and -1 not in (corr_radius_list or ()):
            raise ValueError('return_confidence needs a global matching step (a corr_radius of -1 in corr_radius_list)')
        if fuse_neighbours and task != 'depth':
            raise ValueError("fuse_neighbours fuses the previous frame into the plane sweep: it needs task='depth'")
        if fuse_neighbours and pred_bidir_depth:
            raise ValueError('fuse_neighbours replaces the backward prediction: it cannot be combined with pred_bidir_depth')
        if task == 'depth':
            return self._depth_sequence(frames, attn_type, attn_splits_list, prop_radius_list, num_reg_refine, pred_bidir_flow,
                                        consistency_check, colorize, pairs_per_launch, carry, intrinsics, poses, min_depth, max_depth,
                                        num_depth_candidates, depth_from_argmax, pred_bidir_depth, return_confidence, peak_radius,
                                        bool(fuse_neighbours))
        self._check_bidir_flow(pred_bidir_flow)
        if consistency_check and not pred_bidir_flow:
            raise AssertionError('consistency_check needs pred_bidir_flow=True (as the reference asserts)')
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'frames: expected [T, 3, H, W], got {tuple(frames.shape)}')
        if int(pairs_per_launch) < 1:
            raise ValueError('pairs_per_launch must be >= 1')
        if carry is not None and tuple(carry['frame'].shape[1:]) != tuple(frames.shape[1:]):
            raise ValueError(f'carry holds a {tuple(carry["frame"].shape[2:])} frame, frames are {tuple(frames.shape[2:])}')
        if carry is not None and 'pose' in carry:
            raise ValueError("carry comes from a task='depth' sequence (its features are those of normalised frames)")
        pairs = frames.shape[0] - (0 if carry is not None else 1)
        if pairs < 1:
            raise ValueError('no frame pair: give at least two frames, or one with a carry')
        kw = dict(attn_type=attn_type if attn_type is not None else '', attn_splits_list=attn_splits_list,
                  corr_radius_list=corr_radius_list, prop_radius_list=prop_radius_list, num_reg_refine=num_reg_refine,
                  pred_bidir_flow=pred_bidir_flow, task='flow')
        track = None                                      # chain_flows' (points, alive, stride) of the next chunk
        if track_points is not None:
            track = self._track_start(track_points, carry, frames)
        assert len(attn_splits_list) == len(corr_radius_list) == len(prop_radius_list) == self.num_scales
        import contextlib
        from . import video
        if interpolate:
            from . import interp
        dev = frames.device
        ops = self.ops
        if frames.is_cuda:
            self.check_parameter_dtypes()
        if self.check_weights:
            self._check_weight_print()
        if frames.is_cuda and self.check_range and getattr(ops, 'mode', 1) == 0:
            from . import _abi
            _abi.check_operand_range('an earlier forward of this process: ')
        guard = torch.cuda.device(dev) if frames.is_cuda else contextlib.nullcontext()
        step = int(pairs_per_launch)
        out = {k: [] for k in ('flow', 'flow_bwd', 'occ_fwd', 'occ_bwd', 'flow_rgb', 'flow_bwd_rgb', 'tracks', 'tracks_visible',
                               'frames_between')}
        confs = []                                        # per chunk: the matching step's confidence dict
        with guard, torch.no_grad():
            prev = None                                   # per-scale features [1, C, h, w] of the frame before frames[i]
            before = None                                 # that frame itself: the first image of the next chunk's first pair
            if carry is not None:
                if self._carry_valid(carry, frames):
                    prev = carry['features']
                    before = carry['frame'].to(dev)
                else:                                     # stale: the stored frame is encoded with the first chunk
                    frames = torch.cat([carry['frame'].to(dev), frames], 0)
            i = 0                                         # first frame of the next chunk's new frames
            while i < frames.shape[0] - (1 if prev is None else 0):
                # the chunk's frames: [prev] + the new ones -- B + 1 frames for B pairs, the first one carried when it was encoded already
                new = frames[i:i + step + (1 if prev is None else 0)]
                feats = self._encode((new,))
                chunk = [([] if prev is None else [p]) + [f] for p, f in zip(prev or feats, feats)]
                nb = new.shape[0] - (1 if prev is None else 0)
                i += new.shape[0]
                conf = {} if return_confidence else None
                pred = self._match_pairs(chunk, nb, kw, confidence=conf)
                if conf is not None:
                    confs.append({k: v if k in ('scale', 'mutual') else v[:nb] for k, v in conf.items()})
                prev = [f[f.shape[0] - 1:] for f in feats]
                fwd = pred[:nb]
                out['flow'].append(fwd)
                occ_f = None
                if pred_bidir_flow:
                    bwd = pred[nb:]
                    out['flow_bwd'].append(bwd)
                    if consistency_check or track is not None or interpolate:
                        occ_f, occ_b = video.forward_backward_consistency_check(fwd, bwd)
                    if consistency_check:
                        out['occ_fwd'].append(occ_f)
                        out['occ_bwd'].append(occ_b)
                if track is not None:
                    trk, vis = video.chain_flows(fwd, occ_f, *track)
                    out['tracks'].append(trk)
                    out['tracks_visible'].append(vis)
                    track = (trk[-1], vis[-1], 1)
                if interpolate:
                    seen = new if before is None else torch.cat([before, new], 0)      # the chunk's nb + 1 frames
                    out['frames_between'].append(interp.interpolate_frames(
                        seen[:-1].float().contiguous(), seen[1:].float().contiguous(), fwd, bwd, interp.between_times(interpolate),
                        occ_fwd=occ_f, occ_bwd=occ_b))
                before = new[new.shape[0] - 1:]
                if colorize:
                    out['flow_rgb'].append(video.flow_to_image(fwd))
                    if pred_bidir_flow:
                        out['flow_bwd_rgb'].append(video.flow_to_image(bwd))
            last = frames[frames.shape[0] - 1:]
            result = {k: v[0] if len(v) == 1 else torch.cat(v, 0) for k, v in out.items() if v}
            if confs:
                result['match_confidence'] = {k: confs[0][k] if k == 'scale' else torch.cat([c[k] for c in confs], 0) for k in confs[0]}
            result['carry'] = {'features': [p.clone() for p in prev], 'frame': last.clone(), 'state': self._carry_state(frames)}
            if track is not None:
                result['carry']['track'] = {'points': track[0].clone(), 'alive': track[1].clone()}
        return result

    @staticmethod
    def _track_start(track_points, carry, frames):
        """``(points, alive, stride)`` for :func:`video.chain_flows` on the first chunk: the carried tracks when the carry holds some
        (``track_points`` then only enables tracking), else the start ``track_points`` names."""
        n = None
        if torch.is_tensor(track_points):
            if track_points.dim() != 2 or track_points.shape[1] != 2 or not track_points.is_floating_point():
                raise ValueError(f'track_points: expected a floating-point [N, 2] tensor of (x, y), got {tuple(track_points.shape)} '
                                 f'{track_points.dtype}')
            n = track_points.shape[0]
        elif track_points != 'dense' and (isinstance(track_points, bool) or not isinstance(track_points, int) or track_points < 1):
            raise ValueError(f"track_points: expected 'dense', an int stride >= 1 or an [N, 2] tensor, got {track_points!r}")
        if carry is not None and 'track' in carry:
            points, alive = carry['track']['points'].to(frames.device), carry['track']['alive'].to(frames.device)
            if n is not None and n != points.shape[0]:
                raise ValueError(f'track_points: {n} points, the carry follows {points.shape[0]}')
            return points, alive, 1
        if n is not None:
            return track_points.to(frames.device).float(), None, 1
        return None, None, 1 if track_points == 'dense' else int(track_points)

    def _depth_sequence(self, frames, attn_type, attn_splits_list, prop_radius_list, num_reg_refine, pred_bidir_flow, consistency_check,
                        colorize, pairs_per_launch, carry, intrinsics, poses, min_depth, max_depth, num_depth_candidates,
                        depth_from_argmax, pred_bidir_depth, return_confidence=False, peak_radius=1, fuse_neighbours=False):
        """:meth:`forward_sequence` for ``task='depth'`` (documented there).  Frame j of the call -- the carried frame first, when
        there is a carry -- has pose ``pose_all[j]`` and intrinsics ``k_all[j]``; pair j is frames (j, j + 1).  ``fuse_neighbours``:
        ``nbr`` is the pair before the next chunk's first one as ``_match`` left it (tokens, relative pose, intrinsics row) or None."""
        # what forward (_forward_one) asserts for depth
        assert not pred_bidir_flow, 'pred_bidir_flow is a flow option'
        assert not consistency_check, 'consistency_check is a flow option (it needs pred_bidir_flow)'
        assert self.num_scales == 1
        assert len(attn_splits_list) == len(prop_radius_list) == self.num_scales == 1
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'frames: expected [T, 3, H, W], got {tuple(frames.shape)}')
        if int(pairs_per_launch) < 1:
            raise ValueError('pairs_per_launch must be >= 1')
        if poses is None or intrinsics is None:
            raise ValueError("task='depth' needs poses [T, 4, 4] (absolute camera-to-world) and intrinsics [1, 3, 3] or [T, 3, 3]")
        count = frames.shape[0]
        if poses.dim() != 3 or tuple(poses.shape) != (count, 4, 4):
            raise ValueError(f'poses: expected [{count}, 4, 4] (one per frame), got {tuple(poses.shape)}')
        if intrinsics.dim() != 3 or tuple(intrinsics.shape[1:]) != (3, 3) or intrinsics.shape[0] not in (1, count):
            raise ValueError(f'intrinsics: expected [1, 3, 3] or [{count}, 3, 3], got {tuple(intrinsics.shape)}')
        if carry is not None:
            if 'pose' not in carry:
                raise ValueError("carry comes from a task='flow' sequence: it holds no pose")
            if tuple(carry['frame'].shape[1:]) != tuple(frames.shape[1:]):
                raise ValueError(f'carry holds a {tuple(carry["frame"].shape[2:])} frame, frames are {tuple(frames.shape[2:])}')
        if count - (0 if carry is not None else 1) < 1:
            raise ValueError('no frame pair: give at least two frames, or one with a carry')
        kw = dict(attn_type=attn_type if attn_type is not None else '', attn_splits_list=attn_splits_list, corr_radius_list=None,
                  prop_radius_list=prop_radius_list, num_reg_refine=num_reg_refine, pred_bidir_flow=False, task='depth',
                  min_depth=min_depth, max_depth=max_depth, num_depth_candidates=num_depth_candidates,
                  depth_from_argmax=depth_from_argmax, pred_bidir_depth=pred_bidir_depth)
        import contextlib
        from . import visualize
        dev = frames.device
        ops = self.ops
        if frames.is_cuda:
            self.check_parameter_dtypes()
        if self.check_weights:
            self._check_weight_print()
        if frames.is_cuda and self.check_range and getattr(ops, 'mode', 1) == 0:
            from . import _abi
            _abi.check_operand_range('an earlier forward of this process: ')
        guard = torch.cuda.device(dev) if frames.is_cuda else contextlib.nullcontext()
        step = int(pairs_per_launch)
        out = {k: [] for k in ('depth', 'depth_bwd', 'depth_rgb', 'depth_bwd_rgb')}
        confs = []                                        # per chunk: the plane sweep's confidence dict, forward direction
        if return_confidence:
            kw['peak_radius'] = peak_radius
        with guard, torch.no_grad():
            pose_all = poses.to(dev).float()
            k_all = intrinsics.to(dev).float().expand(count, 3, 3)
            prev = None
            nbr = None
            if carry is not None:
                pose_all = torch.cat([carry['pose'].to(dev), pose_all], 0)
                k_all = torch.cat([carry['intrinsics'].to(dev), k_all], 0)
                if self._carry_valid(carry, frames):
                    prev = carry['features']
                    if fuse_neighbours:                   # None in a carry made without the flag: a first frame, source 1 off
                        nbr = carry.get('neighbour')
                else:                                     # stale: the stored frame is encoded with the first chunk
                    frames = torch.cat([carry['frame'].to(dev), frames], 0)
            if hasattr(ops, 'relative_pose_pairs') and pose_all.is_cuda:   # every pair of the call in one launch, no sync
                rel = ops.relative_pose_pairs(pose_all)
            else:
                rel = torch.linalg.inv(pose_all[1:]) @ pose_all[:-1]
            i, done = 0, 0                                # first new frame / first pair of the next chunk
            while i < frames.shape[0] - (1 if prev is None else 0):
                new = frames[i:i + step + (1 if prev is None else 0)]
                feats = self._encode((new,), 'depth')
                chunk = [([] if prev is None else [p]) + [f] for p, f in zip(prev or feats, feats)]
                nb = new.shape[0] - (1 if prev is None else 0)
                i += new.shape[0]
                conf = {} if return_confidence else None
                neighbour = {'carry': nbr, 'out': None} if fuse_neighbours else None
                pred = self._match_pairs(chunk, nb, kw, k_all[done:done + nb], rel[done:done + nb], confidence=conf, neighbour=neighbour)
                if fuse_neighbours:
                    nbr = neighbour['out']
                if conf is not None:
                    confs.append({k: v[:nb] if torch.is_tensor(v) else v for k, v in conf.items()})
                done += nb
                prev = [f[f.shape[0] - 1:] for f in feats]
                fwd = pred[:nb]
                out['depth'].append(fwd)
                if pred_bidir_depth:
                    bwd = pred[nb:]
                    out['depth_bwd'].append(bwd)
                if colorize:
                    out['depth_rgb'].append(visualize.inverse_depth_to_image(fwd))
                    if pred_bidir_depth:
                        out['depth_bwd_rgb'].append(visualize.inverse_depth_to_image(bwd))
            last = frames[frames.shape[0] - 1:]
            result = {k: v[0] if len(v) == 1 else torch.cat(v, 0) for k, v in out.items() if v}
            if confs:
                result['depth_confidence'] = {k: torch.cat([c[k] for c in confs], 0) if torch.is_tensor(confs[0][k]) else confs[0][k]
                                              for k in confs[0]}
            result['carry'] = {'features': [p.clone() for p in prev], 'frame': last.clone(), 'state': self._carry_state(frames),
                               'pose': pose_all[-1:].clone(), 'intrinsics': k_all[-1:].clone()}
            if fuse_neighbours:
                result['carry']['neighbour'] = nbr
        return result

    def _match_pairs(self, chunk, nb, kw, intrinsics=None, pose=None, confidence=None, neighbour=None):
        """The match step (task ``kw['task']``) of the ``nb`` pairs of consecutive frames whose features are ``chunk[s]`` (per scale, a
        list of pieces ``[N_i, C, h, w]`` that together hold the ``nb + 1`` frames in order) -> predictions ``[bidir * nb, ...]`` in the
        reference's [forward; backward] order.  The stream ``[F[lo:hi]; F[lo+1:hi+1]]`` of pairs lo .. hi-1 is ONE concatenation per
        scale.  ``intrinsics [nb, 3, 3]``, ``pose [nb, 4, 4]`` (depth): per pair, sliced with the features.  Where
        ``streams.forward_parts`` says so, the pairs run as concurrent parts on the process-wide side streams (``streams.PartRunner``);
        with ``confidence`` (the dict ``_match`` fills) or ``neighbour`` (``_match``: the previous pair as a second source of every
        sweep, which ties each pair to the one before it) they run as one part."""
        def frames_of(pieces, a, b):                  # the pieces that hold frames a .. b-1 of the chunk
            out, base = [], 0
            for t in pieces:
                lo, hi = max(a, base), min(b, base + t.shape[0])
                if lo < hi:
                    out.append(t[lo - base:hi - base])
                base += t.shape[0]
            return out

        def stream(lo, hi):
            return [torch.cat(frames_of(pieces, lo, hi) + frames_of(pieces, lo + 1, hi + 1), 0) for pieces in chunk]

        def rows(t, lo, hi):
            return None if t is None else t[lo:hi]

        ref = chunk[-1][-1]
        h8, w8 = ref.shape[-2:]
        parts = self._plan_parts(self.launch_parts, kw['task'], kw['attn_type'], nb, self.upsample_factor * h8, self.upsample_factor * w8,
                                 ref.is_cuda)
        if parts <= 1 or confidence is not None or neighbour is not None:
            more = {} if neighbour is None else {'neighbour': neighbour}
            return self._match(stream(0, nb), nb, intrinsics=intrinsics, pose=pose, confidence=confidence, **more, **kw)['flow_preds'][0]

        def prepare(r):
            lo, hi = shard_bounds(nb, r, parts)
            return stream(lo, hi), hi - lo, rows(intrinsics, lo, hi), rows(pose, lo, hi)

        def compute(r, ins):
            return self._match(ins[0], ins[1], intrinsics=ins[2], pose=ins[3], **kw)['flow_preds']

        bidir = 2 if (kw['pred_bidir_flow'] or kw.get('pred_bidir_depth')) else 1
        return self._runner.run_parts(self, parts, nb, bidir, (nb,) + tuple(ref.shape[1:]), ref.device, kw, prepare,
                                      compute)['flow_preds'][0]

    def _forward_one(self, img0, img1, attn_type=None, attn_splits_list=None, corr_radius_list=None,
                     prop_radius_list=None, num_reg_refine=1, pred_bidir_flow=False, task='flow', intrinsics=None,
                     pose=None, min_depth=1. / 0.5, max_depth=1. / 10, num_depth_candidates=64,
                     depth_from_argmax=False, pred_bidir_depth=False, pred_out=None, confidence=None, peak_radius=1):
        """One forward of the given samples on the current stream.  ``pred_out``: a contiguous ``[B, 2, H, W]`` tensor the flow
        prediction may be written to (it is then the returned prediction; a path that cannot do so ignores it)."""
        self._check_bidir_flow(pred_bidir_flow)
        if pred_bidir_flow:
            assert task == 'flow'
        if task == 'depth':
            assert self.num_scales == 1
            assert len(attn_splits_list) == len(prop_radius_list) == self.num_scales == 1
        else:
            assert len(attn_splits_list) == len(corr_radius_list) == len(prop_radius_list) == self.num_scales
        ops = self.ops
        if img0.is_cuda:
            self.check_parameter_dtypes()
        if self.check_weights:
            self._check_weight_print()
        attn_type = attn_type if attn_type is not None else ''
        dev = img0.device
        # Operand range of exact mode (include/unimatch_hip.h): the kernels raise a sticky flag in pinned host memory when an
        # activation >= 65504 is turned into an fp16 operand.  Reading it costs no synchronisation, so it is read HERE, at the start
        # of every forward: an overflow of an earlier (finished) forward is reported loudly instead of living on as NaN predictions;
        # `check_operand_range()` synchronises first and covers the call that has just been made.
        if img0.is_cuda and self.check_range and getattr(ops, 'mode', 1) == 0:
            from . import _abi
            _abi.check_operand_range('an earlier forward of this process: ')

        # every launch of the library goes to torch's CURRENT stream and scratch buffers are allocated on the current device:
        # make the inputs' device current for the whole forward (a model on cuda:1 called while cuda:0 is current)
        import contextlib
        guard = torch.cuda.device(dev) if img0.is_cuda else contextlib.nullcontext()
        if img1.device != dev:
            raise ValueError(f'img0 is on {dev} and img1 on {img1.device}')
        with guard, torch.no_grad():
            # the position table goes into the encoder's last convolution where the encoder's output has one reader, the
            # `stream=both + pos` branch of _match: one scale (no warp, no bidirectional stacking), no refinement (its ori0 / ori1 are
            # position-free), no taps
            with_pos = (self.num_scales == 1 and not self.reg_refine and self.debug_taps is None and getattr(ops, 'fused_glue', False)
                        and self.backbone.takes_raw_images(ops, img0) and img0.shape == img1.shape)
            pos = (lambda h, w: self._position(h, w, attn_splits_list[0], dev)) if with_pos else None
            feats = self._encode((img0, img1), task, pos)
            return self._match(feats, img0.shape[0], stream_has_pos=with_pos, pred_out=pred_out, attn_type=attn_type, attn_splits_list=attn_splits_list,
                               corr_radius_list=corr_radius_list, prop_radius_list=prop_radius_list, num_reg_refine=num_reg_refine,
                               pred_bidir_flow=pred_bidir_flow, task=task, intrinsics=intrinsics, pose=pose, min_depth=min_depth,
                               max_depth=max_depth, num_depth_candidates=num_depth_candidates, depth_from_argmax=depth_from_argmax,
                               pred_bidir_depth=pred_bidir_depth, confidence=confidence, peak_radius=peak_radius)

    def _encode(self, images, task='flow', position=None):
        """The encode step: the CNN encoder of the images of the tuple ``images``, stacked in that order -> per-scale feature maps
        ``[N, C, h, w]``, low -> high resolution.  Strictly per image (InstanceNorm is per sample): a frame's features are the same
        whichever pair asks for them.  ``position(h, w)``: the Transformer's position table, added by the encoder's last launch --
        only for a caller whose one reader of the features wants them with it (``_forward_one``)."""
        ops = self.ops
        input_norm = None
        if task == 'flow':                  # stereo / depth loaders normalise already (unimatch.py:122-124)
            if self.backbone.takes_raw_images(ops, images[0]):
                input_norm = (_IMAGENET_MEAN, _IMAGENET_STD)            # folded into the stem's image packing
            else:
                mean, std = self._constants(images[0].device)
                images = tuple((im / 255. - mean) / std for im in images)
        # two tensors of one size reach the channels-last stem as they are (it reads every pixel once anyway); every other case -- one
        # tensor, three or more (video), the CPU and the NCHW paths -- is stacked here
        pair = (len(images) == 2 and getattr(ops, 'fused_glue', False) and self.backbone.takes_raw_images(ops, images[0])
                and images[0].shape == images[1].shape and images[0].dtype == images[1].dtype == torch.float32
                and images[0].device == images[1].device)
        stack = images[0] if len(images) == 1 else tuple(images) if pair else torch.cat(images, 0)
        if position is not None:
            return self.backbone(stack, ops, input_norm, out_addend=position)[::-1]
        return self.backbone(stack, ops, input_norm)[::-1]              # low -> high resolution

    def _match(self, feats, nb, attn_type='', attn_splits_list=None, corr_radius_list=None, prop_radius_list=None, num_reg_refine=1,
               pred_bidir_flow=False, task='flow', intrinsics=None, pose=None, min_depth=1. / 0.5, max_depth=1. / 10,
               num_depth_candidates=64, depth_from_argmax=False, pred_bidir_depth=False, stream_has_pos=False, pred_out=None,
               confidence=None, peak_radius=1, sources=0, use=None, neighbour=None):
        """The match step: everything after the encoder, on per-scale features ``feats[s] = [f0; f1]`` (``[2 nb, C, h, w]``, the
        first images of the ``nb`` pairs, then the second ones).  ``stream_has_pos``: the encoder added the position table already
        (``_forward_one`` decides; one scale, no refinement).  ``pred_out``: see ``_forward_one``.  ``confidence``: a dict that receives
        ``confidence.match_confidence`` of the tokens the global matching step (``corr_radius == -1``) matches or, for depth,
        ``confidence.depth_match_confidence`` of the plane sweep (window ``peak_radius``), whose launch then also writes the prediction.
        ``sources`` >= 1 (depth, one scale): the ``nb = sources * B`` pairs are ``B`` reference frames with ``sources`` source views each,
        source-major (``intrinsics`` / ``pose`` likewise); the views vote in ONE plane sweep (``um_depth_corr_softmax_multi``; ``use
        [sources, B]`` switches views off per sample) and everything after it runs on the primary pairs, the rows ``[:B]``.
        ``neighbour`` (depth, one scale, the ``nb`` pairs are CONSECUTIVE: pair t is frames (t, t + 1)): a dict ``{'carry': the pair
        before pair 0 or None, 'out': None}``.  Pair t - 1 is then a second source of every sweep -- ``(tok1[t-1], tok0[t-1], inverse
        cam of pair t-1)`` next to ``(tok0[t], tok1[t], cam of pair t)`` -- in ONE ``um_depth_corr_softmax_multi_rows`` launch that reads
        the Transformer's output in place through :meth:`_neighbour_rows`; everything after the sweep sees what it sees without it.
        ``'out'`` receives the last pair (``'tokens' [2, h*w, C]`` = its tok0 | tok1 rows, cloned, ``'pose'``, ``'intrinsics'``)."""
        ops = self.ops
        dev = feats[0].device
        flow, pred = None, None
        if sources:
            assert task == 'depth' and self.num_scales == 1 and not pred_bidir_depth and nb % sources == 0
        if neighbour is not None:
            assert task == 'depth' and self.num_scales == 1 and not pred_bidir_depth and not sources
        for s in range(self.num_scales):
            m0, m1 = feats[s][:nb], feats[s][nb:]                         # [B, C, h, w]
            both = None
            if pred_bidir_flow and s > 0:
                m0, m1 = torch.cat([m0, m1], 0), torch.cat([m1, m0], 0)
                ori0, ori1 = _to_tokens(m0), _to_tokens(m1)               # pre-position, pre-warp tokens
            else:
                both = _to_tokens(feats[s])                               # the encoder's batched output is [f0; f1]
                ori0, ori1 = both[:nb], both[nb:]
            h, w = m0.shape[-2:]
            up = self.upsample_factor * 2 ** (self.num_scales - 1 - s)
            if task == 'depth':
                k_cur = intrinsics.clone()
                k_cur[:, :2] = k_cur[:, :2] / up
            if s > 0:
                if hasattr(ops, 'flow_upsample2x') and flow.is_cuda:
                    flow = ops.flow_upsample2x(flow, 2.0)          # unimatch.py:162-163 on um_flow_upsample2x
                else:
                    flow = F.interpolate(flow, scale_factor=2, mode='bilinear', align_corners=True) * 2
            tok1 = ori1
            if flow is not None:
                assert task != 'depth'
                disp = torch.cat([-flow, torch.zeros_like(flow)], 1) if task == 'stereo' else flow
                if hasattr(ops, 'flow_warp') and ori1.is_cuda:
                    tok1 = ops.flow_warp(ori1, disp.contiguous(), h, w)
                else:
                    tok1 = _to_tokens(_warp(m1, disp))
            splits, prop_r = attn_splits_list[s], prop_radius_list[s]
            pos = self._position(h, w, splits, dev)
            if self.debug_taps is not None:
                self.debug_taps[f'backbone0_s{s}'], self.debug_taps[f'backbone1_s{s}'] = m0, m1
            if tok1 is ori1 and both is not None:
                # no warp, no bidirectional stacking: the stream [f0; f1] is the encoder's output -- one position add on
                # the whole of it instead of two adds and a concatenation
                tok0, tok1 = self.transformer(ops, None, None, h, w, attn_type, splits, stream=both if stream_has_pos else both + pos)
            else:
                assert not stream_has_pos
                tok0, tok1 = self.transformer(ops, ori0 + pos, tok1 + pos, h, w, attn_type, splits)
            if self.debug_taps is not None:
                self.debug_taps[f'f0_s{s}'], self.debug_taps[f'f1_s{s}'] = _to_map(tok0, h, w), _to_map(tok1, h, w)

            # ---- matching layer
            if task == 'depth':
                cand = self._depth_candidates(min_depth, max_depth, num_depth_candidates, dev)
                f0c, f1c = tok0, tok1
                if pred_bidir_depth:
                    f0c, f1c = torch.cat([tok0, tok1], 0), torch.cat([tok1, tok0], 0)
                if neighbour is not None:
                    flow_pred, cam = self._sweep_neighbours(ops, tok0, tok1, h, w, intrinsics, pose, up, cand.contiguous(), neighbour,
                                                            depth_from_argmax, confidence, peak_radius)
                elif hasattr(ops, 'depth_cam') and tok0.is_cuda:   # K / up, K^-1, (inverse) pose packed on the device, no sync
                    cam = ops.depth_cam(intrinsics, pose, float(up), pred_bidir_depth)
                else:
                    kc, pc = k_cur, pose
                    if pred_bidir_depth:
                        kc = k_cur.repeat(2, 1, 1)
                        pc = torch.cat([pose, torch.inverse(pose)], 0)
                    cam = torch.cat([torch.inverse(kc).flatten(1), pc[:, :3, :3].flatten(1), pc[:, :3, 3],
                                     kc.flatten(1)], 1).float().contiguous()
                if neighbour is not None:
                    pass                                           # swept above, with the cam pack
                elif sources:
                    b = nb // sources
                    flow_pred = self._sweep_multiview(ops, tok0, tok1, h, w, cam, cand.contiguous(), sources, use, depth_from_argmax, up,
                                                      confidence, peak_radius)
                    # propagation, upsampling and refinement run on the primary pair of every reference frame, as in forward
                    tok0, ori0, ori1, cam = tok0[:b], ori0[:b], ori1[:b], cam[:b]
                    intrinsics, pose, k_cur = intrinsics[:b], pose[:b], k_cur[:b]
                elif confidence is not None:
                    flow_pred, conf = depth_match_confidence(ops, f0c, f1c, h, w, cam, cand.contiguous(), depth_from_argmax, up, peak_radius)
                    confidence.update(conf)
                else:
                    flow_pred = ops.depth_corr_softmax(f0c, f1c, h, w, cam, cand.contiguous(), depth_from_argmax)
            else:
                radius = corr_radius_list[s]
                if radius == -1:
                    if confidence is not None and task in ('flow', 'stereo'):
                        confidence.update(match_confidence(tok0, tok1, h, w, task, pred_bidir_flow, up, getattr(ops, 'precision', 'exact')))
                    if task == 'flow':
                        flow_pred = ops.global_corr_softmax_flow(tok0, tok1, h, w, pred_bidir_flow)
                    elif task == 'stereo':
                        flow_pred = ops.global_corr_softmax_stereo(tok0, tok1, h, w)
                    else:
                        raise NotImplementedError
                else:
                    if task not in ('flow', 'stereo'):
                        raise NotImplementedError
                    flow_pred = ops.local_corr_softmax(tok0, tok1, h, w, radius, one_d=(task == 'stereo'))
            flow = flow_pred if flow is None else flow + flow_pred
            if task == 'stereo':
                flow = flow.clamp(min=0)
            if self.debug_taps is not None:
                self.debug_taps[f'flow_match_s{s}'] = flow

            # ---- propagation
            if (pred_bidir_flow or pred_bidir_depth) and s == 0:
                tok0 = torch.cat([tok0, tok1], 0)
            flow = self.feature_flow_attn(ops, tok0, flow.contiguous(), h, w,
                                          local_window_attn=prop_r > 0, local_window_radius=prop_r)
            if self.debug_taps is not None:
                self.debug_taps[f'flow_prop_s{s}'] = flow
            if s < self.num_scales - 1:
                continue

            # ---- full-resolution prediction
            f0_map = _to_map(tok0, h, w)
            if not self.reg_refine:
                if task == 'stereo':
                    pad = torch.cat([-flow, torch.zeros_like(flow)], 1)
                    pred = -self._upsample(pad, f0_map)[:, :1]
                elif task == 'depth':
                    pad = torch.cat([flow, torch.zeros_like(flow)], 1)
                    pred = self._upsample(pad, f0_map, is_depth=True).clamp(min=min_depth, max=max_depth)[:, :1]
                else:
                    pred = self._upsample(flow, f0_map, out=pred_out)
                continue
            assert num_reg_refine > 0
            pose_r = pose
            nhwc = None                                     # channels-last refinement block on the library's convolutions
            if getattr(ops, 'fused_conv', False) and tok0.is_cuda:      # every task: flow_dim 2 (flow) / 1 (disparity, inverse depth)
                nhwc = NhwcUpdateBlock(ops, self.refine, self.refine_proj)
                nhwc.begin(tok0, tok0.shape[0], h, w, iterations=num_reg_refine)
            else:
                proj = self.refine_proj(f0_map)             # same every iteration (unimatch.py:315-320)
                net0, inp = torch.tanh(proj[:, :128]), torch.relu(proj[:, 128:])
            for it in range(num_reg_refine):
                if task == 'stereo':
                    disp = torch.cat([-flow, torch.zeros_like(flow)], 1)
                elif task == 'depth':
                    if pred_bidir_depth and it == 0:
                        ori0, ori1 = torch.cat([ori0, ori1], 0), torch.cat([ori1, ori0], 0)
                    if hasattr(ops, 'rigid_flow') and flow.is_cuda:     # geometry.py:99-195 on um_rigid_flow (cam from the matching layer)
                        disp = ops.rigid_flow(flow, cam)
                    else:
                        if pred_bidir_depth and it == 0:
                            k_cur = k_cur.repeat(2, 1, 1)
                            pose_r = torch.cat([pose, torch.inverse(pose)], 0)
                        disp = _rigid_flow(1. / flow.squeeze(1), k_cur, pose_r)
                else:
                    disp = flow
                if nhwc is not None:
                    up_mask, delta = nhwc.iterate(ori0, ori1, disp.contiguous(), flow, it == num_reg_refine - 1)
                else:
                    corr = ops.local_corr_with_flow(ori0, ori1, disp.contiguous(), h, w, 4)
                    _, up_mask, delta = self.refine(net0, inp, corr, flow)
                if task == 'depth':
                    flow = (flow - delta).clamp(min=min_depth, max=max_depth)
                else:
                    flow = flow + delta
                if task == 'stereo':
                    flow = flow.clamp(min=0)
                if self.debug_taps is not None:
                    self.debug_taps[f'flow_it{it}'] = flow
                if it == num_reg_refine - 1:
                    if task == 'depth':
                        pad = torch.cat([flow, torch.zeros_like(flow)], 1)
                        pred = self._upsample(pad, f0_map, is_depth=True).clamp(
                            min=min_depth, max=max_depth)[:, :1]
                    elif nhwc is not None:
                        pred = ops.convex_upsample(flow, up_mask, self.upsample_factor, False, mask_nhwc=True,
                                                   out=pred_out if task == 'flow' and not pred_bidir_flow else None)
                    else:
                        pred = self._convex(flow, up_mask)
        if task == 'stereo':
            pred = pred.squeeze(1)
        if task == 'depth':
            pred = 1. / pred.squeeze(1)
        return {'flow_preds': [pred]}
