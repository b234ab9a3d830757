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


def confidence_to_image(max_prob, size):
    """``max_prob [B, h, w]`` nearest-upsampled to ``size = (H, W)`` and coloured per image (min-max, inferno) through
    ``visualize.scalar_to_image`` (``um_scalar_to_rgb`` on the device): ``[B, H, W, 3]`` uint8."""
    from .visualize import scalar_to_image
    up = torch.nn.functional.interpolate(max_prob[:, None].float(), size=tuple(size), mode='nearest')[:, 0]
    return scalar_to_image(up.contiguous(), 'inferno')
