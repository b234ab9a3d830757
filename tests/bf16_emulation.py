"""As-rounded host emulation of the bf16 ('fast') instantiations of the matching-path kernels.  TEST INFRASTRUCTURE ONLY.

Plain torch on the host.  Every emulation takes ``dtype`` (torch.float64 or torch.float32) and ``rounding``:

  ``True``        round to bf16 exactly where the ``<Bf16, 1, ...>`` instantiation does (operands AND the in-kernel points);
  ``'operands'``  round the operands only: the "truth on rounded operands" T of the issue -- E64 - T is the rounding noise of the
                  in-kernel points alone;
  ``False``       no rounding at all: the function then IS the oracle / the fp64 expression of the exact-mode test.

All other arithmetic is in ``dtype``.  ``rb`` is torch's round-to-nearest-even conversion, which is what ``Bf16::down`` and
``Bf16::pack2`` (csrc/common.h:85-96) compile to.

Rounding points of the fast mode (file:line of unimatch_amd/csrc), as read from the kernels:

  operands       fp32 -> one bf16 plane, after the factor the plane carries: split_planes / split_elems (scale first, then
                 T::pack2); tokens read by a kernel itself: linear.hip:123, ffn.hip:353 (kv4), ffn.hip:472 (FFN), window_attn.hip:374
                 (q-projection prologue).  Weight planes carry 2^wshift (a power of two: does not move the rounding); the planes of
                 global_match.hip carry um_global_corr_plane_scale(C) = sqrt(log2(e) / sqrt(C)) on both sides (global_match.hip:1153-1154,
                 1233-1234), which does.
  window attn    p = exp2(fma(s, c, M)), M an integer offset (window_attn.hip:683); the row sum adds the UNROUNDED p (:685); P is
                 packed for P.V (:700).  The value operand is the v plane.  Integer M: the rounding of p does not depend on the
                 offset the kernel held, so -ceil(row maximum) serves.
  q prologue     q = acc * 2^-wshift is packed (window_attn.hip:407-409).
  merge epilogue message = O / l is packed for the Wm product (window_attn.hip:1009-1011); LayerNorm and residual in fp32.
  linear         plane outputs are packed after out_scale, bias and GELU (linear.hip:194-202, 234, 238); the LayerNorm and fp32
                 epilogues round nothing (linear.hip:206-218, 259-297).
  FFN            gelu(hidden) is packed for the W2 product (ffn.hip:569); LayerNorm + fp32 residual after it round nothing.
  kv4            the four outputs are planes (ffn.hip:318-321); inside um_ffn_kv_fwd the normalised tile is packed exactly as the
                 stand-alone kernel packs the tokens it reads (ffn.hip:1149-1150).
  gsv3 / gsv4    NOTHING but the operand planes: the scores leave the MFMAs in fp32, p = exp2(score) stays fp32 and P.V is a chain
                 of fp32 FMAs on values loaded as fp32 by vload (global_match.hip:261-264, 272-282; 694-697, 718-739) in both
                 instantiations; the combine kernels are fp32 (global_match.hip:945-1000).  Pixel coordinates are therefore exact.

``gate`` is the one acceptance function shared by the GPU parity file and by the host-only self test.
"""
import torch
import torch.nn.functional as F

from oracle import hotpath as hp

U = 2.0 ** -8            # largest relative error of one round-to-nearest bf16 conversion (8 significant bits)
EPS32 = 2.0 ** -23
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def rb(x):
    return x.bfloat16().to(x.dtype)


def _op(x, dtype, rounding):
    """An operand plane: fp32 input, rounded once (in fp32, as the device does)."""
    return (rb(x) if rounding else x).to(dtype)


def _mid(x, rounding):
    """An in-kernel rounding point."""
    return rb(x) if rounding is True else x


# ------------------------------------------------------------------------------------------------ the gate
def gate(got, e64, e32, bound=None, floor=0.0, what=''):
    """The acceptance test of one fast-mode output ``got`` against its as-rounded emulations; returns the measured figures.

    (a) finite; (b) every element within ``bound + floor`` of E64 (``bound``: what two independent roundings at the kernel's
    rounding points can move the output by, ``None`` where the kernel rounds nothing; ``floor``: the absolute tolerance of the same
    kernel's exact-mode test); (c) mean|got - E64| <= 8 mean|E32 - E64| + 4 fp32 ulps of mean|E64| -- the right-hand side is
    measured from the reference alone."""
    got, e64, e32 = got.detach().double().cpu(), e64.double(), e32.double()
    assert got.shape == e64.shape == e32.shape, (what, got.shape, e64.shape, e32.shape)
    assert torch.isfinite(got).all(), (what, 'not finite')
    d = (got - e64).abs()
    ref = (e32 - e64).abs()
    lim = floor if bound is None else bound.double() + floor
    over = d - lim
    stats = {'got_mean': d.mean().item(), 'got_max': d.max().item(), 'ref_mean': ref.mean().item(), 'ref_max': ref.max().item()}
    stats['rhs'] = 8.0 * stats['ref_mean'] + 4.0 * EPS32 * e64.abs().mean().item()
    stats['ratio'] = stats['got_mean'] / max(stats['ref_mean'], 1e-300)
    assert (over <= 0).all(), (what, 'element bound', over.max().item(), stats)
    assert stats['got_mean'] <= stats['rhs'], (what, 'mean gate', stats)
    return stats


def exact_close(a, b, rel=1e-12):
    """rounding=False reduces to the oracle: equal to ``rel`` of the output scale."""
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() <= rel * max(1.0, b.abs().max().item())


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln(z, gamma, beta, eps):
    return F.layer_norm(z, (z.shape[-1],), gamma.to(z.dtype), beta.to(z.dtype), eps)


def _ln_bound(z, dz, gamma, eps):
    """|d LayerNorm(z)| for |dz| <= ``dz`` elementwise.  With zh = (z - mean) / sigma:
    d zh_n = (dz_n - mean(dz)) / sigma - zh_n * mean(zh * dz) / sigma, so
    |dy_n| <= |gamma_n| / sigma * (dz_n + mean(dz) + |zh_n| mean(|zh| dz)); first order, +5 % for the second-order terms
    (dz / sigma stays below 2^-5 in every case of the suite, so they are below 2^-5 of the bound)."""
    mu = z.mean(-1, keepdim=True)
    sig = ((z - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    zh = (z - mu) / sig
    b = (dz + dz.mean(-1, keepdim=True) + zh.abs() * (zh.abs() * dz).mean(-1, keepdim=True)) / sig
    return 1.05 * gamma.to(z.dtype).abs() * b


# ------------------------------------------------------------------------------------------------ window attention
def _attn_core(q, k, v, h, w, win_h, win_w, shift_h, shift_w, rounding, kv_rotate=0, key_mult=None, want_bound=False):
    """q, k, v: operand planes as ``[S, L, C]`` tensors of the working dtype.  -> out, sum_j p_j |v_j| / sum_j p_j (or None).
    ``key_mult`` ``[n]``: how often each key of a window is counted (1 everywhere: no defect)."""
    s, l, c = q.shape
    dtype = q.dtype
    idx, label = hp.window_index(h, w, win_h, win_w, shift_h, shift_w)
    nwin, n = idx.shape
    flat = idx.reshape(-1)
    mask = None
    if shift_h > 0 or shift_w > 0:
        neq = label[:, :, None] != label[:, None, :]
        mask = torch.zeros(nwin, n, n, dtype=dtype).masked_fill_(neq, hp.MASK_NEG)
    out = torch.empty_like(q)
    absb = torch.empty_like(q) if want_bound else None
    mult = None if key_mult is None else key_mult.to(dtype).view(1, 1, n)
    for i in range(s):
        j = (i + kv_rotate) % s                                  # stream i reads the keys / values of stream (i + r) mod S
        qw, kw, vw = q[i, flat].view(nwin, n, c), k[j, flat].view(nwin, n, c), v[j, flat].view(nwin, n, c)
        logit = torch.bmm(qw, kw.transpose(1, 2)) / (c ** 0.5)
        if mask is not None:
            logit = logit + mask
        # one arithmetic for every ``rounding``: switched off, only _mid becomes the identity, so that the comparison with the
        # oracle covers the exp2 form, the integer offset and the separate row sum
        t = logit * LOG2E
        p = torch.exp2(t - torch.ceil(t.max(-1, keepdim=True).values))           # integer offset: window_attn.hip:665, 683
        if mult is not None:
            p = p * mult
        lsum = p.sum(-1, keepdim=True)                             # the row sum adds the unrounded p: window_attn.hip:685
        pp = _mid(p, rounding)                                     # P packed for P.V: window_attn.hip:700
        o = torch.bmm(pp, vw) / lsum
        ab = torch.bmm(pp, vw.abs()) / lsum if want_bound else None
        out[i, flat] = o.reshape(nwin * n, c)
        if want_bound:
            absb[i, flat] = ab.reshape(nwin * n, c)
    return out, absb


def window_attention(q, k, v, h, w, win_h, win_w, shift_h, shift_w, dtype, rounding=True, key_mult=None, want_bound=False):
    """um_window_attn_fwd.  rounding=False: oracle.hotpath.window_attention.
    -> out, or (out, bound) with bound = 2 U sum_j p_j |v_j| / sum_j p_j (each packed probability is off by at most U relative,
    once in the kernel and once here)."""
    out, ab = _attn_core(_op(q, dtype, rounding), _op(k, dtype, rounding), _op(v, dtype, rounding), h, w, win_h, win_w,
                         shift_h, shift_w, rounding, key_mult=key_mult, want_bound=want_bound)
    return (out, 2.0 * U * ab) if want_bound else out


def attention_merge(qp, kp, vp, wm, norm, residual, streams, h, w, win_h, win_w, shift_h, shift_w, kv_rotate, dtype,
                    rounding=True, want_bound=False, merge=True):
    """um_window_attn_planes_fwd (``merge=False``) / um_window_attn_merge_fwd / the part of um_window_attn_qproj_merge_fwd behind
    its prologue.  ``qp, kp, vp``: the operand PLANES as float tensors ``[S*L, C]`` (already rounded: outputs of ``linear``);
    ``norm`` = (gamma, beta, eps).  rounding=False: LayerNorm(window_attention(q, k, v) . Wm^T) (+ residual).
    -> (attention output, merged layer output) from one pass over the windows; each a (value, bound) pair with ``want_bound``.
    Bound: d message_c <= 2 U sum p|v| / sum p + 2 U |message_c| (P, then the packing of the message at window_attn.hip:1011),
    d z_n <= sum_c |Wm_nc| d message_c, then ``_ln_bound``."""
    c = qp.shape[-1]
    sh = (streams, h * w, c)
    o, ab = _attn_core(qp.to(dtype).view(sh), kp.to(dtype).view(sh), vp.to(dtype).view(sh), h, w, win_h, win_w, shift_h, shift_w,
                       rounding, kv_rotate=kv_rotate, want_bound=want_bound)
    o = o.view(-1, c)
    attn = (o, 2.0 * U * ab.view(-1, c)) if want_bound else o
    if not merge:
        return attn
    msg = _mid(o, rounding)                                       # window_attn.hip:1009-1011
    wmo = _op(wm, dtype, rounding)
    z = msg @ wmo.t()
    gamma, beta, eps = norm
    out = _ln(z, gamma, beta, eps)
    if residual is not None:
        out = out + residual.to(dtype)
    if not want_bound:
        return attn, out
    dm = 2.0 * U * ab.view(-1, c) + 2.0 * U * msg.abs()
    return attn, (out, _ln_bound(z, dm @ wmo.abs().t(), gamma, eps))


# ------------------------------------------------------------------------------------------------ um_linear_fwd family
def linear(a, w, dtype, rounding=True, a1=None, gelu=False, bias=None, out_mul=1.0, bias_mul=1.0, out='planes', norm=None,
           residual=None, a_is_planes=False):
    """um_linear_fwd / um_linear_bias_fwd / the q-projection prologue: ``(A . W^T) * out_mul + bias * bias_mul``, then
    out='planes': (GELU,) packed to bf16 (linear.hip:234-238; window_attn.hip:407-409); out='f32': nothing; out='ln':
    LayerNorm (+ residual), nothing rounded.  ``a_is_planes``: A already is a plane (values representable in bf16)."""
    if a1 is not None:
        a = torch.cat([a, a1], 1)
    ao = a.to(dtype) if a_is_planes else _op(a, dtype, rounding)
    acc = ao @ _op(w, dtype, rounding).t()
    if out_mul != 1.0:
        acc = acc * out_mul
    if bias is not None:
        acc = acc + bias.to(dtype) * bias_mul
    if gelu:
        acc = F.gelu(acc)
    if out == 'planes':
        return _mid(acc, rounding)
    if out == 'ln':
        gamma, beta, eps = norm
        acc = _ln(acc, gamma, beta, eps)
        if residual is not None:
            acc = acc + residual.to(dtype)
    return acc


def planes_bound(e64):
    """An output plane: the kernel and the emulation round accumulators that differ by fp32 noise; where that noise straddles a
    rounding boundary the two results are one bf16 spacing apart, at most 2 U |E64|."""
    return 2.0 * U * e64.abs()


def ffn(x, y, w1, w2, norm, dtype, rounding=True, hidden_mult=None, want_bound=False):
    """um_ffn_fwd / um_ffn_ws_fwd: x + LayerNorm(W2 . gelu(W1 . [x | y])); gelu(hidden) is packed (ffn.hip:569), x is added as
    fp32.  ``hidden_mult`` ``[hidden]``: how often each hidden unit is counted (defects).
    Bound: d z_n <= 2 U sum_h |g_h| |W2_nh|, then ``_ln_bound``."""
    hid = torch.cat([_op(x, dtype, rounding), _op(y, dtype, rounding)], 1) @ _op(w1, dtype, rounding).t()
    g = _mid(F.gelu(hid), rounding)
    if hidden_mult is not None:
        g = g * hidden_mult.to(dtype)
    w2o = _op(w2, dtype, rounding)
    z = g @ w2o.t()
    gamma, beta, eps = norm
    out = x.to(dtype) + _ln(z, gamma, beta, eps)
    if not want_bound:
        return out
    return out, _ln_bound(z, 2.0 * U * (g.abs() @ w2o.abs().t()), gamma, eps)


def kv4(x, ws, dtype, rounding=True):
    """um_kv4_fwd: four 128 x 128 projections of one token stream as planes -> ``[4, M, 128]``."""
    return torch.stack([linear(x, w_, dtype, rounding) for w_ in ws], 0)


# ------------------------------------------------------------------------------------------------ global matching
def _plane(f, ps, dtype, rounding):
    """The global-matching operand plane of tokens f: bf16(f * ps), the factor BEFORE the rounding (global_match.hip:1153)."""
    return rb(f.float() * ps).to(dtype) if rounding else f.to(dtype)             # the product is an fp32 product on the device


def _gsv_probs(q, k, ps, dtype, rounding, causal=False, key_mult=None):
    """softmax over the keys of q . k^T.  Rounded planes carry ps each, so their product is the logit in log2 units; unrounded
    operands take the oracle's q . k / sqrt(C)."""
    c = q.shape[-1]
    if rounding:
        logit = torch.matmul(_plane(q, ps, dtype, True), _plane(k, ps, dtype, True).transpose(-1, -2)) * LN2
    else:
        logit = torch.matmul(q.to(dtype), k.to(dtype).transpose(-1, -2)) / (c ** 0.5)
    if causal:
        n = logit.shape[-1]
        xs = torch.arange(n)
        logit = logit.masked_fill(xs[None, :] > xs[:, None], hp.OOB_NEG)
    if key_mult is None:
        return torch.softmax(logit, -1)
    p = torch.exp(logit - logit.max(-1, keepdim=True).values) * key_mult.to(dtype)
    return p / p.sum(-1, keepdim=True)


def global_matching(f0, f1, h, w, ps, dtype, rounding=True, values=(), stereo=True, bidir=True, key_mult=None):
    """um_global_corr_softmax_flow (both directions), um_global_corr_softmax_stereo and um_prop_global_attn(q = f0 tokens,
    k = f1 tokens, value) from ONE score matrix.  f0, f1: tokens ``[B, L, C]``; values: maps ``[B, V, h, w]``.
    The kernels round nothing but the planes (see the module docstring), so rounding=True and 'operands' coincide;
    rounding=False is oracle.hotpath.global_corr_softmax_flow / _stereo and softmax(q k^T / sqrt C) . value.
    ``key_mult`` ``[L, L]`` (query, key): how often a key is counted for a query in the forward direction (defects)."""
    b, l, c = f0.shape
    grid = hp.pixel_grid(h, w, dtype).flatten(1).t()                                   # [L, 2], fp32-exact coordinates
    out = {}
    prob = _gsv_probs(f0, f1, ps, dtype, rounding, key_mult=key_mult)
    fwd = (prob @ grid - grid).transpose(1, 2).reshape(b, 2, h, w)
    out['props'] = [(prob @ v.to(dtype).flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, -1, h, w) for v in values]
    del prob
    if bidir:
        prob = _gsv_probs(f1, f0, ps, dtype, rounding)
        bwd = (prob @ grid - grid).transpose(1, 2).reshape(b, 2, h, w)
        del prob
        out['flow'] = torch.cat([fwd, bwd], 0)
    else:
        out['flow'] = fwd
    if stereo:
        r0, r1 = f0.view(b, h, w, c), f1.view(b, h, w, c)
        prob = _gsv_probs(r0, r1, ps, dtype, rounding, causal=True)                    # [B, h, w, w']
        xg = torch.arange(w, dtype=dtype)
        out['stereo'] = (xg.view(1, 1, w) - (prob * xg).sum(-1)).unsqueeze(1)
    return out


def prop_projected(x, wq, bq, wk, bk, value, h, w, ps, dtype, rounding=True, planes=None):
    """HipOps.prop_global_projected: q = Wq x + bq and k = Wk q + bk through um_linear_bias_fwd as planes carrying ps
    (out_mul / bias_mul are applied BEFORE the pack: linear.hip:194-202, 238), then um_prop_global_attn_planes.
    ``planes`` = (qp, kp) as float tensors: take these (the device's own) planes for the attention stage.
    rounding=False: softmax((Wq x + bq)(Wk q + bk)^T / sqrt C) . value.  -> out, (qp, kp)."""
    b, l, c = x.shape
    xs = x.reshape(b * l, c)
    if rounding:
        if planes is None:
            qp = linear(xs, wq, dtype, rounding, bias=bq, out_mul=ps, bias_mul=ps)
            kp = linear(qp, wk, dtype, rounding, bias=bk, out_mul=1.0, bias_mul=ps, a_is_planes=True)
        else:
            qp, kp = (p.to(dtype) for p in planes)
        logit = torch.bmm(qp.view(b, l, c), kp.view(b, l, c).transpose(1, 2)) * LN2
    else:
        qp = linear(xs, wq, dtype, False, bias=bq, out='f32')
        kp = linear(qp, wk, dtype, False, bias=bk, out='f32')
        logit = torch.bmm(qp.view(b, l, c), kp.view(b, l, c).transpose(1, 2)) / (c ** 0.5)
    prob = torch.softmax(logit, -1)
    out = (prob @ value.to(dtype).flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, -1, h, w)
    return out, (qp, kp)


def plane_scale(c=128):
    """um_global_corr_plane_scale(C) as the library computes it: fp32 sqrt of fp32 (log2(e) / sqrtf(C)) (global_match.hip:1039, 1257).
    The GPU file asserts that the library returns this very number."""
    s = torch.tensor(LOG2E, dtype=torch.float32) / torch.tensor(float(c), dtype=torch.float32).sqrt()
    return float(s.sqrt())
