"""Matching confidence: statistics of every row of the global matching distribution, without forming it.

The reference's matching layer returns the distribution next to the flow -- ``global_correlation_softmax`` gives ``(flow, prob)``
(unimatch/matching.py:7-36), ``global_correlation_softmax_stereo`` ``(disparity, prob)`` (matching.py:126-151) -- and the fused kernels
of this library never form it.  With ``p_ij = softmax_j(q_i . k_j / sqrt(C))`` over all keys (flow) or over the keys ``x' <= x`` of
the query's scanline (stereo):

  global_match_stats(f0, f1, h, w, bidir=, stereo=, precision=)   ``MatchStats`` of every query: ``max_prob = max_j p_ij``,
                                                                  ``best = argmax_j p_ij`` (token index ``y*w + x`` for flow, column
                                                                  ``x'`` for stereo, lowest index on a tie), ``entropy = -sum p ln p``
                                                                  (nats), ``variance = sum_j p_ij |g_j - mu_i|^2`` in feature pixels^2
                                                                  (2-D for flow, x only for stereo) and ``mean = mu_i - g_i``: the flow,
                                                                  or minus the disparity, the matching entry points return
  mutual_matches(best_fwd, best_bwd, h, w, radius=0)              bool ``[B, h, w]``: ``best_bwd[best_fwd[i]]`` lies within ``radius``
                                                                  feature pixels of ``i`` in x and y (0: mutual nearest neighbours)

CUDA tensors run ``um_global_match_stats`` / ``um_match_mutual`` (csrc/match_stats.hip); host tensors run the ``*_host`` restatements
below, plain torch that forms ``prob`` and follows the dtype of its inputs (the tests evaluate it in float64).  There is no silent
fallback from one to the other.

Depth has its own distribution: the plane sweep's ``match_prob [B, D, h, w]`` over the D inverse-depth candidates of a pixel
(``correlation_softmax_depth`` gives ``(depth, match_prob)``, matching.py:203-236), which the sweep's kernels reduce to one number.

  depth_match_stats(f0, f1, h, w, cam, candidates, peak_radius=)  ``DepthMatchStats`` of every pixel: ``max_prob``, ``entropy``, ``variance =
                                                                  sum_j p_j (c_j - mu)^2`` about the soft-argmin ``mu`` (inverse depth^2),
                                                                  ``peak_mass`` = the probability within ``peak_radius`` candidates of
                                                                  ``best`` (the first arg-max candidate), ``in_view`` = candidates with
                                                                  a bilinear corner inside the image (0: all logits 0, uniform)
  depth_match_confidence(ops, ...)                                the sweep's prediction and the ``'depth_confidence'`` dict of
                                                                  ``UniMatch.forward_with_depth_confidence``
  confidence_to_image_size(map, scale, geom)                      a feature-resolution map at image size

CUDA tensors run ``um_depth_corr_softmax_stats`` (csrc/local_ops.hip: the sweep's own launch also writes the statistics); host tensors
run ``depth_match_prob_host`` / ``depth_stats_from_prob_host``, the reference's ``match_prob`` from the packed camera record.

  depth_match_multi(f0, f1, h, w, cam, candidates, use=)          several source views ``[S, B, ...]`` vote in one sweep: the logits are
                                                                  averaged over the sources that see a candidate, then one softmax
                                                                  (``um_depth_corr_softmax_multi``; unlearned, the weights know two views);
                                                                  ``rows=``: the operands are rows of other tensors, named by a table
                                                                  and not copied (``um_depth_corr_softmax_multi_rows``)
"""
from collections import namedtuple

import torch

from . import _abi

MatchStats = namedtuple('MatchStats', 'max_prob entropy variance best mean')
MatchStats.__doc__ = ('``max_prob``, ``entropy``, ``variance`` ``[B\', h, w]`` float, ``best`` ``[B\', h, w]`` int32, ``mean`` '
                      '``[B\', 2 or 1, h, w]``; ``B\' = 2B`` with ``bidir`` (the second half is ``f1 -> f0``).')

_PRECISIONS = {'exact': _abi.MODE_EXACT, 'fast': _abi.MODE_FAST}


def _check_features(f0, f1, h, w):
    if f0.dim() != 3 or f1.shape != f0.shape or f0.shape[1] != h * w or f1.dtype != f0.dtype or f1.device != f0.device:
        raise ValueError(f'expected two [B, h*w = {h * w}, C] feature tensors of one shape, dtype and device, got '
                         f'{tuple(f0.shape)} {f0.dtype} {f0.device} and {tuple(f1.shape)} {f1.dtype} {f1.device}')


# ------------------------------------------------------------------ host restatement
def match_prob_host(f0, f1, h, w, stereo=False):
    """The reference's ``prob``: ``[B, h*w, h*w]`` (flow) or ``[B, h, w, w]`` with the keys ``x' > x`` at zero (stereo)."""
    b, l, c = f0.shape
    if stereo:
        corr = f0.view(b, h, w, c) @ f1.view(b, h, w, c).transpose(-1, -2) / c ** 0.5
        right = torch.triu(torch.ones(w, w, dtype=torch.bool, device=f0.device), diagonal=1)
        return torch.softmax(corr.masked_fill(right, float('-inf')), -1)
    return torch.softmax(f0 @ f1.transpose(-1, -2) / c ** 0.5, -1)


def stats_from_prob_host(prob, h, w, stereo=False):
    """``MatchStats`` of a given ``prob`` (as :func:`match_prob_host` lays it out), in its dtype."""
    dt, dev = prob.dtype, prob.device
    b = prob.shape[0]
    max_prob, best = prob.max(-1)                                      # the first maximal index, as the kernel
    plogp = torch.where(prob > 0, prob * torch.log(prob.clamp(min=torch.finfo(dt).tiny)), torch.zeros_like(prob))
    entropy = -plogp.sum(-1)
    x = torch.arange(w, dtype=dt, device=dev)
    if stereo:
        d = x.view(1, 1, 1, w) - x.view(1, 1, w, 1)                    # key - query
        mean = (prob * d).sum(-1)
        variance = (prob * (d - mean[..., None]) ** 2).sum(-1)
        mean = mean.view(b, 1, h, w)
    else:
        gx, gy = x.repeat(h), torch.arange(h, dtype=dt, device=dev).repeat_interleave(w)
        dx, dy = gx.view(1, 1, -1) - gx.view(1, -1, 1), gy.view(1, 1, -1) - gy.view(1, -1, 1)
        mx, my = (prob * dx).sum(-1), (prob * dy).sum(-1)
        variance = (prob * ((dx - mx[..., None]) ** 2 + (dy - my[..., None]) ** 2)).sum(-1)
        mean = torch.stack([mx, my], 1).view(b, 2, h, w)
    return MatchStats(max_prob.reshape(b, h, w), entropy.reshape(b, h, w), variance.clamp(min=0).reshape(b, h, w),
                      best.reshape(b, h, w).to(torch.int32), mean)


def global_match_stats_host(f0, f1, h, w, bidir=False, stereo=False):
    """:func:`global_match_stats` as a plain torch composition that forms ``prob``, in the dtype and on the device of the inputs."""
    _check_features(f0, f1, h, w)
    if bidir and stereo:
        raise ValueError('bidir is a flow option: the stereo distribution runs over the keys left of the query only')
    if bidir:
        f0, f1 = torch.cat([f0, f1], 0), torch.cat([f1, f0], 0)
    return stats_from_prob_host(match_prob_host(f0, f1, h, w, stereo), h, w, stereo)


def mutual_matches_host(best_fwd, best_bwd, h, w, radius=0):
    b = best_fwd.shape[0]
    l = h * w
    fwd, bwd = best_fwd.reshape(b, l).long(), best_bwd.reshape(b, l).long()
    ok = (fwd >= 0) & (fwd < l)
    back = bwd.gather(1, fwd.clamp(0, l - 1))
    ok = ok & (back >= 0) & (back < l)
    back = back.clamp(0, l - 1)
    i = torch.arange(l, device=fwd.device).view(1, l)
    cheb = torch.maximum((back % w - i % w).abs(), (back // w - i // w).abs())
    return (ok & (cheb <= radius)).view(b, h, w)


# ------------------------------------------------------------------ public functions
def global_match_stats(f0, f1, h, w, *, bidir=False, stereo=False, precision='exact'):
    """``MatchStats`` of the matching distribution of the token-major features ``f0``, ``f1`` ``[B, h*w, 128]``.  ``bidir`` (flow
    only) appends the ``f1 -> f0`` direction; ``stereo`` matches per scanline over the keys ``x' <= x`` (a query at ``x = 0`` has one
    key: exactly ``max_prob = 1, entropy = 0, variance = 0``).  ``precision``: the operand format of the kernel, ``'exact'`` (fp16
    hi | lo) or ``'fast'`` (bf16); the host restatement follows its inputs' dtype instead."""
    _check_features(f0, f1, h, w)
    if precision not in _PRECISIONS:
        raise ValueError(f'precision must be one of {sorted(_PRECISIONS)}')
    if bidir and stereo:
        raise ValueError('bidir is a flow option: the stereo distribution runs over the keys left of the query only')
    if not f0.is_cuda:
        return global_match_stats_host(f0, f1, h, w, bidir, stereo)
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    if not (f0.dtype == torch.float32 and f0.is_contiguous() and f1.is_contiguous()):
        raise ValueError(f'expected contiguous CUDA float32 features, got {f0.dtype} contiguous={f0.is_contiguous()}, {f1.is_contiguous()}')
    b, l, c = f0.shape
    mode = _PRECISIONS[precision]
    nb = 2 * b if bidir else b
    with torch.cuda.device(f0.device):
        stats = torch.empty((nb, 3, h, w), dtype=torch.float32, device=f0.device)
        best = torch.empty((nb, h, w), dtype=torch.int32, device=f0.device)
        mean = torch.empty((nb, 1 if stereo else 2, h, w), dtype=torch.float32, device=f0.device)
        ws = torch.empty(max(int(lib.um_global_match_stats_workspace_bytes(b, l, c, mode)), 256), dtype=torch.uint8, device=f0.device)
        _abi.check(lib.um_global_match_stats(f0.data_ptr(), f1.data_ptr(), stats.data_ptr(), best.data_ptr(), mean.data_ptr(), b, h, w, c,
                                             int(bool(bidir)), int(bool(stereo)), mode, ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream), 'um_global_match_stats')
    return MatchStats(stats[:, 0], stats[:, 1], stats[:, 2], best, mean)


def mutual_matches(best_fwd, best_bwd, h, w, radius=0):
    """bool ``[B, h, w]``: query ``i`` and its best key agree, ``best_bwd[b, best_fwd[b, i]]`` lies within ``radius`` feature pixels
    of ``i`` in both x and y.  ``best_fwd``, ``best_bwd``: ``[B, h, w]`` token indices (the two halves of a ``bidir`` ``best``)."""
    if best_fwd.shape != best_bwd.shape or best_fwd.dim() != 3 or tuple(best_fwd.shape[1:]) != (h, w) or best_bwd.device != best_fwd.device:
        raise ValueError(f'expected two [B, {h}, {w}] index maps on one device, got {tuple(best_fwd.shape)} and {tuple(best_bwd.shape)}')
    if int(radius) < 0:
        raise ValueError(f'radius must be >= 0, got {radius}')
    if not best_fwd.is_cuda:
        return mutual_matches_host(best_fwd, best_bwd, h, w, int(radius))
    lib = _abi.load()
    fwd, bwd = best_fwd.to(torch.int32).contiguous(), best_bwd.to(torch.int32).contiguous()
    with torch.cuda.device(fwd.device):
        out = torch.empty(fwd.shape, dtype=torch.uint8, device=fwd.device)
        _abi.check(lib.um_match_mutual(fwd.data_ptr(), bwd.data_ptr(), out.data_ptr(), fwd.shape[0], h, w, int(radius),
                                       torch.cuda.current_stream().cuda_stream), 'um_match_mutual')
    return out.bool()


def match_confidence(tok0, tok1, h, w, task, bidir, scale, precision='exact'):
    """The ``'match_confidence'`` dict of ``UniMatch.forward_with_confidence`` from the tokens the flow is matched on."""
    s = global_match_stats(tok0.contiguous(), tok1.contiguous(), h, w, bidir=bidir, stereo=(task == 'stereo'), precision=precision)
    out = {'max_prob': s.max_prob, 'entropy': s.entropy, 'variance': s.variance, 'best': s.best, 'scale': int(scale)}
    if bidir:
        b = tok0.shape[0]
        out['mutual'] = mutual_matches(s.best[:b], s.best[b:], h, w, 0)
    return out


# ------------------------------------------------------------------ depth: the plane sweep's distribution
DepthMatchStats = namedtuple('DepthMatchStats', 'max_prob entropy variance peak_mass best in_view')
DepthMatchStats.__doc__ = ('Statistics of the plane sweep\'s ``match_prob`` (unimatch/matching.py:227) over the D inverse-depth candidates of '
                           'every pixel: ``max_prob``, ``entropy`` (nats), ``variance`` (about the soft-argmin, inverse depth squared), '
                           '``peak_mass`` (the probability within ``peak_radius`` candidates of the best one) ``[B, h, w]`` float; ``best`` '
                           '(first arg-max candidate) and ``in_view`` (candidates with a bilinear corner inside the image; 0: a uniform '
                           'distribution) ``[B, h, w]`` int32.')


def _check_depth_inputs(f0, f1, h, w, cam, candidates):
    _check_features(f0, f1, h, w)
    if tuple(cam.shape) != (f0.shape[0], 30) or cam.device != f0.device:
        raise ValueError(f'cam: expected [{f0.shape[0]}, 30] = K^-1 | R | t | K on {f0.device}, got {tuple(cam.shape)} on {cam.device}')
    if candidates.dim() != 1 or not 1 <= candidates.numel() <= 128 or candidates.device != f0.device:
        raise ValueError(f'candidates: expected 1 .. 128 inverse depths [D] on {f0.device}, got {tuple(candidates.shape)} on {candidates.device}')


def depth_sample_coords_host(h, w, cam, candidates):
    """Where every candidate of every pixel lands in the second view: ``(sx, sy)`` ``[B, D, h, w]`` in feature pixels, in ``cam``'s dtype
    and in the kernel's operation order (back-project, rotate, scale by depth, translate, project, clamp ``z >= 1e-3``)."""
    dt, dev = cam.dtype, cam.device
    b = cam.shape[0]
    kinv, rot, trans, k = cam[:, 0:9].view(b, 3, 3), cam[:, 9:18].view(b, 3, 3), cam[:, 18:21], cam[:, 21:30].view(b, 3, 3)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=dt, device=dev), torch.arange(w, dtype=dt, device=dev), indexing='ij')

    def mat(m, x, y, z):                                                   # rows of m [B, 3, 3] times (x, y, z), left to right
        return [m[:, i, 0].view(b, 1, 1, 1) * x + m[:, i, 1].view(b, 1, 1, 1) * y + m[:, i, 2].view(b, 1, 1, 1) * z for i in range(3)]

    r = mat(kinv, gx.view(1, 1, h, w), gy.view(1, 1, h, w), torch.ones((), dtype=dt, device=dev))
    q = mat(rot, *r)
    depth = (1.0 / candidates.to(dt)).view(1, -1, 1, 1)
    x, y, z = (q[i] * depth + trans[:, i].view(b, 1, 1, 1) for i in range(3))
    u, v, zz = mat(k, x, y, z)
    zz = zz.clamp(min=1e-3)
    return (u / zz).clamp(-1.0e6, 1.0e6), (v / zz).clamp(-1.0e6, 1.0e6)


def depth_match_logits_host(f0, f1, h, w, cam, candidates):
    """``(logits [B, D, h, w], in_view [B, h, w] int32)`` of the plane sweep: feature1 sampled bilinearly with zero padding where each
    candidate lands, correlated with feature0, over ``sqrt(C)``.  ``in_view`` counts the candidates with a corner inside the image."""
    logits, visible = depth_match_logits_visible_host(f0, f1, h, w, cam, candidates)
    return logits, visible.sum(1).to(torch.int32)


def depth_match_logits_visible_host(f0, f1, h, w, cam, candidates):
    """:func:`depth_match_logits_host` with the per-candidate visibility instead of its count: ``(logits [B, D, h, w], visible
    [B, D, h, w] bool)``, ``visible`` = the candidate has a bilinear corner inside the image (``x0`` in ``[-1, w-1]``, ``y0`` in
    ``[-1, h-1]``)."""
    _check_depth_inputs(f0, f1, h, w, cam, candidates)
    b, l, c = f0.shape
    dt = f0.dtype
    sx, sy = depth_sample_coords_host(h, w, cam.to(dt), candidates)
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    wx, wy = sx - fx0, sy - fy0
    x0, y0 = fx0.long(), fy0.long()
    d = x0.shape[1]
    a = f0.view(b, 1, l, c)
    corr = torch.zeros((b, d, l), dtype=dt, device=f0.device)
    batch = torch.arange(b, device=f0.device).view(b, 1, 1)
    for cy in (0, 1):
        for cx in (0, 1):
            yy, xx = (y0 + cy).view(b, d, l), (x0 + cx).view(b, d, l)
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            wt = ((wx if cx else 1 - wx) * (wy if cy else 1 - wy)).view(b, d, l)
            rows = f1[batch, (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1))]            # [B, D, L, C]
            corr = corr + torch.where(ok, wt * (a * rows).sum(-1), torch.zeros((), dtype=dt, device=f0.device))
    visible = (x0 >= -1) & (x0 < w) & (y0 >= -1) & (y0 < h)
    return (corr / c ** 0.5).view(b, d, h, w), visible


def depth_match_prob_host(f0, f1, h, w, cam, candidates):
    """The reference's ``match_prob`` ``[B, D, h, w]`` (``correlation_softmax_depth``, unimatch/matching.py:203-236) from token-major
    features ``[B, h*w, C]`` and the packed ``cam [B, 30]`` = K^-1 | R | t | K record, in the dtype of the features."""
    return torch.softmax(depth_match_logits_host(f0, f1, h, w, cam, candidates)[0], 1)


def depth_stats_from_prob_host(prob, candidates, in_view, peak_radius):
    """``DepthMatchStats`` of a given ``prob [B, D, h, w]``, in its dtype (``in_view`` is passed through)."""
    if int(peak_radius) < 0:
        raise ValueError(f'peak_radius must be >= 0, got {peak_radius}')
    dt, dev = prob.dtype, prob.device
    d = prob.shape[1]
    max_prob, best = prob.max(1)                                           # the first maximal index, as the kernel
    plogp = torch.where(prob > 0, prob * torch.log(prob.clamp(min=torch.finfo(dt).tiny)), torch.zeros_like(prob))
    entropy = (-plogp.sum(1)).clamp(min=0)
    cand = candidates.to(dt).view(1, d, 1, 1)
    mu = (prob * cand).sum(1, keepdim=True)
    variance = (prob * (cand - mu) ** 2).sum(1)
    j = torch.arange(d, device=dev).view(1, d, 1, 1)
    window = (j - best[:, None]).abs() <= int(peak_radius)
    peak_mass = torch.where(window, prob, torch.zeros_like(prob)).sum(1)   # radius 0: one term and zeros, max_prob exactly
    return DepthMatchStats(max_prob, entropy, variance, peak_mass, best.to(torch.int32), in_view)


def depth_match_stats_host(f0, f1, h, w, cam, candidates, peak_radius=1):
    """:func:`depth_match_stats` as a plain torch composition that forms ``match_prob``, in the dtype and on the device of the inputs."""
    logits, seen = depth_match_logits_host(f0, f1, h, w, cam, candidates)
    return depth_stats_from_prob_host(torch.softmax(logits, 1), candidates, seen, peak_radius)


def depth_match_stats(f0, f1, h, w, cam, candidates, *, peak_radius=1):
    """``DepthMatchStats`` of the plane sweep of the token-major features ``f0``, ``f1`` ``[B, h*w, 128]`` under ``cam [B, 30]`` over the
    inverse-depth ``candidates [D]``.  CUDA tensors run ``um_depth_corr_softmax_stats`` (the sweep's own launch, its prediction
    discarded); host tensors run the restatement above.  There is no fallback from one to the other."""
    _check_depth_inputs(f0, f1, h, w, cam, candidates)
    if int(peak_radius) < 0:
        raise ValueError(f'peak_radius must be >= 0, got {peak_radius}')
    if not f0.is_cuda:
        return depth_match_stats_host(f0, f1, h, w, cam, candidates, int(peak_radius))
    return _depth_sweep_device(f0, f1, h, w, cam, candidates, False, int(peak_radius))[1]


def _depth_sweep_device(f0, f1, h, w, cam, candidates, from_argmax, peak_radius, ops=None):
    """``(out [B, 1, h, w], DepthMatchStats)`` of one ``um_depth_corr_softmax_stats`` launch; through ``ops`` (a ``HipOps``: its launch
    record sees the call) when given."""
    if ops is not None:
        out, stats, index = ops.depth_corr_softmax(f0, f1, h, w, cam, candidates, from_argmax, stats=True, peak_radius=peak_radius)
    else:
        lib = _abi.load()                    # raises when the HIP extension is missing: there is no silent fallback
        tensors = (f0, f1, cam, candidates)
        if not all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
            raise ValueError('expected contiguous CUDA float32 features, cam and candidates')
        b, l, c = f0.shape
        with torch.cuda.device(f0.device):
            out = torch.empty((b, 1, h, w), dtype=torch.float32, device=f0.device)
            stats = torch.empty((b, 4, h, w), dtype=torch.float32, device=f0.device)
            index = torch.empty((b, 2, h, w), dtype=torch.int32, device=f0.device)
            _abi.check(lib.um_depth_corr_softmax_stats(f0.data_ptr(), f1.data_ptr(), cam.data_ptr(), candidates.data_ptr(), out.data_ptr(),
                                                       stats.data_ptr(), index.data_ptr(), b, h, w, c, candidates.numel(),
                                                       int(bool(from_argmax)), int(peak_radius), torch.cuda.current_stream().cuda_stream),
                       'um_depth_corr_softmax_stats')
    return out, DepthMatchStats(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], index[:, 0], index[:, 1])


def depth_match_confidence(ops, f0, f1, h, w, cam, candidates, from_argmax, scale, peak_radius=1):
    """The plane sweep's prediction and the ``'depth_confidence'`` dict of ``UniMatch.forward_with_depth_confidence``:
    ``(out [B, 1, h, w], dict)``.  On the GPU both come from the one fused launch of ``ops``; on host tensors the prediction comes from
    the backend ``ops`` as in :meth:`forward` and the statistics from the host restatement."""
    if int(peak_radius) < 0:
        raise ValueError(f'peak_radius must be >= 0, got {peak_radius}')
    if f0.is_cuda:
        out, s = _depth_sweep_device(f0.contiguous(), f1.contiguous(), h, w, cam, candidates, from_argmax, int(peak_radius), ops)
    else:
        out = ops.depth_corr_softmax(f0, f1, h, w, cam, candidates, from_argmax)
        s = depth_match_stats_host(f0, f1, h, w, cam, candidates, int(peak_radius))
    conf = dict(s._asdict(), scale=int(scale), num_candidates=int(candidates.numel()))
    return out, conf


# ------------------------------------------------------------------ depth: several source views in one plane sweep
def _check_multi_inputs(f0, f1, h, w, cam, candidates, use):
    if f0.dim() != 4 or not 1 <= f0.shape[0] <= 8:
        raise ValueError(f'expected source-major features [S = 1 .. 8, B, h*w, C], got {tuple(f0.shape)}')
    if cam.dim() != 3 or cam.shape[0] != f0.shape[0]:
        raise ValueError(f'cam: expected [{f0.shape[0]}, {f0.shape[1]}, 30], got {tuple(cam.shape)}')
    if f1.shape != f0.shape:
        raise ValueError(f'f1: expected {tuple(f0.shape)}, got {tuple(f1.shape)}')
    for s in range(f0.shape[0]):
        _check_depth_inputs(f0[s], f1[s], h, w, cam[s], candidates)
    if use is not None and (tuple(use.shape) != tuple(f0.shape[:2]) or use.device != f0.device):
        raise ValueError(f'use: expected [{f0.shape[0]}, {f0.shape[1]}] on {f0.device}, got {tuple(use.shape)} on {use.device}')


def depth_rows_to_source_major_host(segments, cam, rows):
    """The operands a row table names, copied into the source-major layout: ``(f0, f1 [S, B, h*w, C], cam [S, B, 30], use [S, B]
    bool)``.  ``segments``: 1 .. 4 token tensors ``[n_i, h*w, C]`` (a token row indexes their concatenation in order), ``cam [Rc, 30]``,
    ``rows [S, B, 3]`` integer = f0 row | f1 row | cam row.  A source with a negative or too-large index is off (``use`` false): its
    operands in the result are placeholders that nothing reads.  Works on any device; on the GPU this copy is what the row-table launch
    exists to avoid."""
    if torch.is_tensor(segments) or not 1 <= len(segments) <= 4:
        raise ValueError('rows: f0 must be a tuple or list of 1 .. 4 token tensors (the segments)')
    if any(t.dim() != 3 or t.shape[1:] != segments[0].shape[1:] or t.shape[0] < 1 or t.dtype != segments[0].dtype
           or t.device != segments[0].device for t in segments):
        raise ValueError(f'segments: expected [n_i >= 1, h*w, C] tensors of one dtype and device, got {[tuple(t.shape) for t in segments]}')
    if cam.dim() != 2 or cam.shape[0] < 1 or cam.shape[1] != 30:
        raise ValueError(f'cam: expected [Rc >= 1, 30] with a row table, got {tuple(cam.shape)}')
    if rows.dim() != 3 or not 1 <= rows.shape[0] <= 8 or rows.shape[2] != 3 or rows.is_floating_point():
        raise ValueError(f'rows: expected integer [S = 1 .. 8, B, 3] = f0 row | f1 row | cam row, got {tuple(rows.shape)} {rows.dtype}')
    tokens = segments[0] if len(segments) == 1 else torch.cat(list(segments), 0)
    idx = rows.long()
    total, cam_rows = tokens.shape[0], cam.shape[0]
    use = (idx >= 0).all(-1) & (idx[..., 0] < total) & (idx[..., 1] < total) & (idx[..., 2] < cam_rows)
    idx = torch.where(use[..., None], idx, torch.zeros_like(idx))
    return tokens[idx[..., 0]], tokens[idx[..., 1]], cam[idx[..., 2]], use


def depth_match_logits_multi_host(f0, f1, h, w, cam, candidates, use=None, rows=None):
    """The fused logits of the multi-view plane sweep (``um_depth_corr_softmax_multi``), in the dtype of the inputs.  ``f0``, ``f1``
    ``[S, B, h*w, C]``, ``cam [S, B, 30]``, ``use [S, B]`` (false: the source is off for that sample and is not read) or None.  With
    ``l_sj`` the logit and ``v_sj`` the visibility of :func:`depth_match_logits_visible_host` for source ``s``:

        ``n_j = sum_s v_sj``,   ``l_j = (sum_s v_sj l_sj) / max(1, n_j)``

    -- a mean over the sources that see the candidate (an unlearned extension: the weights are trained on two views).  Returns
    ``(logits [B, D, h, w], in_view [B, h, w] int32 = candidates with n_j >= 1, views [B, D, h, w] int32 = n_j)``.

    With ``rows [S, B, 3]`` (``um_depth_corr_softmax_multi_rows``): ``f0`` is the tuple or list of segments, ``f1`` None, ``cam [Rc, 30]``;
    the rows are gathered into the source-major layout (:func:`depth_rows_to_source_major_host`) and an off source is ``use`` false."""
    if rows is not None:
        if f1 is not None or use is not None:
            raise ValueError('rows names every operand: f1 must be None (f0 holds the segments) and use must be None')
        f0, f1, cam, use = depth_rows_to_source_major_host(f0, cam, rows)
    _check_multi_inputs(f0, f1, h, w, cam, candidates, use)
    s_count, b = f0.shape[:2]
    d = candidates.numel()
    total = torch.zeros((b, d, h, w), dtype=f0.dtype, device=f0.device)
    views = torch.zeros((b, d, h, w), dtype=torch.int32, device=f0.device)
    on = torch.ones((s_count, b), dtype=torch.bool) if use is None else use.to(torch.bool).cpu()
    for s in range(s_count):
        rows = torch.nonzero(on[s]).flatten().to(f0.device)
        if rows.numel() == 0:
            continue
        logits, visible = depth_match_logits_visible_host(f0[s][rows], f1[s][rows], h, w, cam[s][rows], candidates)
        total[rows] = total[rows] + torch.where(visible, logits, torch.zeros((), dtype=f0.dtype, device=f0.device))
        views[rows] = views[rows] + visible.to(torch.int32)
    fused = total / views.clamp(min=1).to(f0.dtype)
    return fused, (views >= 1).sum(1).to(torch.int32), views


def depth_match_stats_multi_host(f0, f1, h, w, cam, candidates, use=None, peak_radius=1, rows=None):
    """``DepthMatchStats`` of the fused distribution ``softmax_j l_j`` of :func:`depth_match_logits_multi_host`, which it forms."""
    logits, seen, _ = depth_match_logits_multi_host(f0, f1, h, w, cam, candidates, use, rows)
    return depth_stats_from_prob_host(torch.softmax(logits, 1), candidates, seen, peak_radius)


def depth_match_multi(f0, f1, h, w, cam, candidates, use=None, *, from_argmax=False, peak_radius=1, ops=None, rows=None):
    """The multi-view plane sweep: ``(out [B, 1, h, w], DepthMatchStats)`` of the source-major ``f0``, ``f1`` ``[S, B, h*w, 128]`` under
    ``cam [S, B, 30]`` over the inverse-depth ``candidates [D]``; ``use [S, B]`` switches sources off per sample.  ``out`` is the
    soft-argmin of the fused distribution (``from_argmax``: the candidate at ``best``).  CUDA tensors run ONE
    ``um_depth_corr_softmax_multi`` launch (through ``ops``, a ``HipOps``, when given: its launch record sees the call); host tensors
    run the restatement above.  There is no fallback from one to the other.  The fusion is unlearned: see csrc/depth_multi.hip.

    ``rows [S, B, 3]`` int32 = f0 row | f1 row | cam row: the operands are rows of other tensors, named and not copied.  ``f0`` is then
    a tuple or list of 1 .. 4 token tensors ``[n_i, h*w, 128]`` (the segments; a token row indexes their concatenation), ``f1`` and
    ``use`` are None and ``cam`` is ``[Rc, 30]``; a source with a negative or too-large index is off for that sample.  CUDA tensors run
    ONE ``um_depth_corr_softmax_multi_rows`` launch, bit for bit the contiguous launch on the gathered operands; host tensors gather
    the rows and run the same restatement."""
    if int(peak_radius) < 0:
        raise ValueError(f'peak_radius must be >= 0, got {peak_radius}')
    if rows is not None:
        if f1 is not None or use is not None:
            raise ValueError('rows names every operand: f1 must be None (f0 holds the segments) and use must be None')
        if torch.is_tensor(f0) or not 1 <= len(f0) <= 4:
            raise ValueError('rows: f0 must be a tuple or list of 1 .. 4 token tensors (the segments)')
        is_cuda = f0[0].is_cuda
    else:
        _check_multi_inputs(f0, f1, h, w, cam, candidates, use)
        is_cuda = f0.is_cuda
    if not is_cuda:
        logits, seen, _ = depth_match_logits_multi_host(f0, f1, h, w, cam, candidates, use, rows)
        prob = torch.softmax(logits, 1)
        st = depth_stats_from_prob_host(prob, candidates, seen, int(peak_radius))
        cand = candidates.to(prob.dtype)
        out = cand[st.best.long()][:, None] if from_argmax else (prob * cand.view(1, -1, 1, 1)).sum(1, keepdim=True)
        return out, st
    if ops is None:
        from .ops import HipOps              # raises when the HIP extension is missing: there is no silent fallback
        ops = HipOps('exact')
    out, stats, index = ops.depth_corr_softmax(f0, f1, h, w, cam, candidates, from_argmax, stats=True, peak_radius=int(peak_radius), use=use,
                                               **({} if rows is None else {'rows': rows}))
    return out, DepthMatchStats(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], index[:, 0], index[:, 1])


def depth_match_multi_confidence(ops, f0, f1, h, w, cam, candidates, use, from_argmax, scale, peak_radius=1, rows=None):
    """The fused sweep's prediction and its ``'depth_confidence'`` dict (the keys of :func:`depth_match_confidence`); ``rows``: the
    operands by row table, as in :func:`depth_match_multi`."""
    out, s = depth_match_multi(f0, f1, h, w, cam, candidates, use, from_argmax=from_argmax, peak_radius=peak_radius, ops=ops, rows=rows)
    return out, dict(s._asdict(), scale=int(scale), num_candidates=int(candidates.numel()))


def confidence_to_image_size(conf_map, scale, geom=None):
    """A feature-resolution map ``[B, h, w]`` at image size: nearest upsampling by ``scale`` (the dict's stride), then -- with ``geom``,
    the ``prepost.InferenceGeometry`` the images were prepared with -- ``geom.restore(., 'depth')``, which crops or resizes without
    rescaling values.  ``[B, H, W]`` float32."""
    up = torch.nn.functional.interpolate(conf_map[:, None].float(), scale_factor=int(scale), mode='nearest')[:, 0].contiguous()
    return up if geom is None else geom.restore(up, 'depth')


def confidence_to_image(max_prob, size):
    """``max_prob [B, h, w]`` nearest-upsampled to ``size = (H, W)`` and coloured per image (min-max, inferno) through
    ``visualize.scalar_to_image`` (``um_scalar_to_rgb`` on the device): ``[B, H, W, 3]`` uint8."""
    from .visualize import scalar_to_image
    up = torch.nn.functional.interpolate(max_prob[:, None].float(), size=tuple(size), mode='nearest')[:, 0]
    return scalar_to_image(up.contiguous(), 'inferno')
