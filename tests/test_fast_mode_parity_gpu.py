"""Fast-mode (bf16) parity: every ``<Bf16, 1, ...>`` instantiation of the matching path against an fp64 emulation that rounds
where the kernel rounds (tests/bf16_emulation.py), at the exact-mode file's edge shapes -- plus, in both modes, the two production
entry points that had no direct test (HipOps.linear_bias, HipOps.prop_global_projected) and one-channel global propagation.

Per case, ``got`` from HipOps('fast') must pass ``bf16_emulation.gate``:
  (a) finite;
  (b) every element within ``bound + floor`` of E64, the as-rounded fp64 emulation.  ``floor`` is the absolute tolerance of the same
      kernel's exact-mode test (with equal operands fp32 accumulation is all that is left).  ``bound`` follows from the kernel's
      rounding points, each off by at most U = 2^-8 relative, once in the kernel and once in E64:
        attention              2 U sum_j p_j |v_j| / sum_j p_j                                   (P packed for P.V)
        attention + merge      d message_c = (the above) + 2 U |message_c|, d z_n = sum_c |Wm_nc| d message_c, through the LayerNorm:
                               |gamma_n| / sigma (dz_n + mean dz + |zh_n| mean(|zh| dz)) * 1.05   (bf16_emulation._ln_bound)
        FFN                    d z_n = 2 U sum_h |gelu(hidden)_h| |W2_nh|, through the same LayerNorm bound
        bf16-plane outputs     2 U |E64|  (one bf16 spacing where fp32 noise straddles a rounding boundary)
        linear_ln, linear_bias with fp32 output, gsv3 / gsv4 (flow, stereo, propagation): nothing is rounded in the kernel -> floor only
  (c) mean|got - E64| <= 8 mean|E32 - E64| + 4 fp32 ulps of mean|E64|, E32 the same emulation evaluated in fp32 on the host.
Every test prints its ratio mean|got - E64| / mean|E32 - E64|; the table is profiles/fast_mode_parity.txt.

Multi-stage cases (projection -> attention) hand the DEVICE's own bf16 planes of one stage to the emulation of the next, so that a
stage is compared on equal operands; every stage is gated on its own.  The host-only self test (test_bf16_emulation_cpu.py) runs the
same case objects with the E64 planes in that role.
"""
import math

import pytest
import torch

from oracle import hotpath as hp
from tests import bf16_emulation as em
from tests.test_hip_parity_gpu import C, DEV, _random_matching_shapes, _random_window_geometries, rnd, tok
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
PS = em.plane_scale(C)


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


@pytest.fixture(scope='module')
def ops_fast():
    return HipOps('fast')


def _bf(planes, m, n):
    """A one-plane (fast mode) operand tensor as floats on the host."""
    return planes.view(torch.bfloat16).view(-1)[:m * n].view(m, n).float().cpu()


def _scale(t):
    return max(1.0, t.abs().max().item())


def _layer_norm(seed_w, seed_b, c=C):
    """(gamma, beta, eps) and the nn.LayerNorm that carries them."""
    norm = torch.nn.LayerNorm(c)
    if seed_w is not None:
        with torch.no_grad():
            norm.weight.copy_(1 + 0.1 * rnd(seed_w, c))
            norm.bias.copy_(0.1 * rnd(seed_b, c))
    return norm, (norm.weight.detach().clone(), norm.bias.detach().clone(), norm.eps)


def _lib_census(lib, fn):
    from unimatch_amd import _abi
    lib.um_census_enable(1)
    try:
        out = fn()
    finally:
        counts = _abi.census(lib)
        lib.um_census_enable(0)
    return out, counts


def report(case_id, name, dispatch, st):
    print(f'PARITY {case_id} | {name} | {dispatch} | got-E64 mean {st["got_mean"]:.3e} max {st["got_max"]:.3e} | '
          f'E32-E64 mean {st["ref_mean"]:.3e} max {st["ref_max"]:.3e} | ratio {st["ratio"]:.2f}')


class Case:
    """One input set.  ``emulate(dtype, rounding, planes=None, want_bound=False)`` -> (outputs, bounds, planes): dicts by output
    name; ``planes`` are the intermediate operand planes a later stage consumes (given: use these; None: compute them).
    ``oracle()``: the fp64 oracle / exact-mode expression, written independently of the emulation.  ``floor(name, e64)``: the
    exact-mode tolerance.  ``device(ops)`` -> (outputs, planes, dispatch string).  ``rounds``: outputs with an in-kernel rounding."""
    rounds = ()

    def check(self, ops_fast, case_id):
        got, planes, dispatch = self.device(ops_fast)
        e64, bounds, _ = self.emulate(F64, True, planes=planes, want_bound=True)
        e32, _, _ = self.emulate(F32, True, planes=planes)
        assert set(got) == set(e64) == set(e32), (sorted(got), sorted(e64))
        for name in sorted(got):
            st = em.gate(got[name], e64[name], e32[name], bounds.get(name), self.floor(name, e64[name]), (case_id, name))
            report(case_id, name, dispatch, st)


# ------------------------------------------------------------------------------------------------ um_window_attn_fwd
LARGER = [(2, 16, 24, 8, 12, 4, 6, 1.0), (1, 20, 28, 10, 14, 5, 7, 2.0), (2, 32, 48, 16, 24, 8, 12, 1.5), (1, 24, 40, 24, 40, 0, 0, 1.0),
          (2, 6, 60, 1, 30, 0, 15, 2.0), (2, 5, 120, 1, 120, 0, 0, 1.0)]        # test_window_attention_larger_shapes


class WindowAttn(Case):
    rounds = ('out',)

    def __init__(self, kind, case):
        if kind == 'larger':
            s, h, w, wh, ww, sh, sw, scale = case
            self.q, self.k, self.v = (rnd(10 + i, s, h * w, C, scale=scale) for i in range(3))
            self.tol = 5e-5
        elif kind == 'random':
            s, h, w, wh, ww, sh, sw = case
            self.q, self.k, self.v = (rnd(700 + i + h * w, s, h * w, C, scale=1.5) for i in range(3))
            self.tol = 5e-5
        else:        # the forced-rescale input: a spiked key far down the window, the running maximum jumps late (LAG = 8 in bf16)
            s, h, w, wh, ww = 1, 16, 24, 8, 12
            sh, sw = case
            self.q, self.k, self.v = (rnd(20 + i, s, h * w, C) for i in range(3))
            self.k[0, 200] = self.q[0, 10] * 6.0
            self.tol = 1e-4
        self.geom = (h, w, wh, ww, sh, sw)

    def emulate(self, dtype, rounding, planes=None, want_bound=False, key_mult=None):
        r = em.window_attention(self.q, self.k, self.v, *self.geom, dtype, rounding, key_mult=key_mult, want_bound=want_bound)
        return ({'out': r[0]}, {'out': r[1]}, None) if want_bound else ({'out': r}, {}, None)

    def oracle(self):
        return {'out': hp.window_attention(self.q.double(), self.k.double(), self.v.double(), *self.geom)}

    def floor(self, name, e64):
        return self.tol * _scale(e64)

    def device(self, o):
        got, c = _lib_census(o.lib, lambda: o.window_attention(self.q.to(DEV), self.k.to(DEV), self.v.to(DEV), *self.geom))
        assert c['wattn_tile'] == 1 and c['wattn_ksplit'] == 0, c
        return {'out': got}, None, 'wattn_tile'


WATTN_CASES = ([('larger', c) for c in LARGER] + [('random', g) for g in _random_window_geometries(28)] +
               [('rescale', (0, 0)), ('rescale', (4, 6))])


@pytest.mark.parametrize('kind,case', WATTN_CASES)
def test_window_attention_fast(ops_fast, kind, case):
    """um_window_attn_fwd<Bf16, 1>: bound 2 U sum p|v| / sum p + 5e-5 max(1, |E64|) (1e-4 for the forced-rescale input)."""
    WindowAttn(kind, case).check(ops_fast, f'wattn-{kind}-{"x".join(str(x) for x in case)}')


# ------------------------------------------------------------------------------------------------ planes / merge / q-projection + merge
PROLOGUE_GEOS = [(2, 16, 24, 8, 12, 4, 6, 1), (2, 10, 30, 1, 30, 0, 0, 0), (2, 12, 20, 12, 20, 0, 0, 1), (4, 6, 10, 3, 5, 1, 2, 2),
                 (2, 9, 40, 1, 10, 0, 5, 1), (2, 64, 96, 32, 48, 16, 24, 1), (1, 80, 120, 80, 120, 0, 0, 0), (1, 32, 48, 32, 48, 0, 0, 0),
                 (2, 40, 56, 20, 28, 10, 14, 1), (2, 32, 48, 16, 24, 8, 12, 1), (1, 64, 96, 32, 48, 16, 24, 0),
                 (16, 64, 96, 32, 48, 16, 24, 8), (12, 40, 56, 20, 28, 0, 0, 0), (32, 60, 80, 30, 40, 15, 20, 16)]
                 # test_query_projection_prologue_matches_q_planes


class AttnLayer(Case):
    """q | k | v projections (um_linear_fwd planes) -> um_window_attn_planes_fwd, um_window_attn_merge_fwd and
    um_window_attn_qproj_merge_fwd on the device's planes."""
    rounds = ('q_planes', 'kv_planes', 'attn', 'merge', 'qproj_merge')

    def __init__(self, kind, case):
        c = C
        if kind == 'rotate':                          # test_attention_merge_and_kv_rotate
            shifted, residual = case
            s_, h, w = 4, 16, 24
            self.geom, self.rot = (h, w) + ((8, 12, 4, 6) if shifted else (8, 12, 0, 0)), 2
            m = s_ * h * w
            self.x, self.xt = rnd(140, m, c, scale=1.5), rnd(141, m, c, scale=1.5)
            self.wq, self.wk, self.wv, self.wm = (rnd(142 + i, c, c, scale=0.09) for i in range(4))
            self.norm, self.ln = _layer_norm(146, 147)
            self.residual = residual
        elif kind == 'prologue':
            s_, h, w, wh, ww, sh, sw, self.rot = case
            self.geom = (h, w, wh, ww, sh, sw)
            m = s_ * h * w
            self.x, self.xt = rnd(900 + h, m, c, scale=1.5), rnd(901 + w, m, c, scale=1.5)
            self.wq, self.wk, self.wv, self.wm = (rnd(902 + i, c, c, scale=0.09) for i in range(4))
            self.norm, self.ln = _layer_norm(None, None)
            self.residual = True
        else:                                         # test_key_split_launches_skip_masked_tiles_too: batch-1 config-2 geometry
            s_, h, w, wh, ww, sh, sw = case
            self.geom, self.rot = (h, w, wh, ww, sh, sw), 0
            self.x = self.xt = rnd(1500, h * w, c, scale=1.5)
            self.wq, self.wk, self.wv, self.wm = (rnd(1501 + i, c, c, scale=0.09) for i in range(4))
            self.norm, self.ln = _layer_norm(None, None)
            self.residual = True
        self.kind, self.streams = kind, s_

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        q = em.linear(self.x, self.wq, dtype, rounding)
        kv = em.linear(self.xt, torch.cat([self.wk, self.wv], 0), dtype, rounding)
        out = {'q_planes': q, 'kv_planes': kv}
        bounds = {}
        qp, kvp = planes if (rounding and planes is not None) else (q, kv)     # later stages: the given (device / E64) planes
        kp, vp = kvp[:, :C], kvp[:, C:]
        res = self.x if self.residual else None
        a, mg = em.attention_merge(qp, kp, vp, self.wm, self.ln, res, self.streams, *self.geom, self.rot, dtype, rounding, want_bound)
        if want_bound:
            bounds = {'q_planes': em.planes_bound(q), 'kv_planes': em.planes_bound(kv), 'attn': a[1], 'merge': mg[1],
                      'qproj_merge': mg[1]}
            a, mg = a[0], mg[0]
        out.update(attn=a, merge=mg, qproj_merge=mg)
        return out, bounds, (q, kv)

    def oracle(self):
        s_, (h, w) = self.streams, self.geom[:2]
        l = h * w
        q64 = (self.x.double() @ self.wq.double().t())
        kv64 = self.xt.double() @ torch.cat([self.wk, self.wv], 0).double().t()
        src = self.xt.double().view(s_, l, C).roll(-self.rot, 0)
        att = hp.window_attention(q64.view(s_, l, C), src @ self.wk.double().t(), src @ self.wv.double().t(), *self.geom)
        g, b, eps = self.ln
        want = torch.nn.functional.layer_norm(att.reshape(s_ * l, C) @ self.wm.double().t(), (C,), g.double(), b.double(), eps)
        if self.residual:
            want = want + self.x.double()
        return {'q_planes': q64, 'kv_planes': kv64, 'attn': att.reshape(s_ * l, C), 'merge': want, 'qproj_merge': want}

    def floor(self, name, e64):
        # planes: test_linear_planes_and_gelu; attention: test_window_attention_*; merged layer: test_attention_merge_and_kv_rotate
        return {'q_planes': 2e-5 * _scale(e64), 'kv_planes': 2e-5 * _scale(e64), 'attn': 5e-5 * _scale(e64)}.get(name, 5e-5)

    def device(self, o):
        import ctypes
        s_, (h, w) = self.streams, self.geom[:2]
        geo = self.geom[2:]
        m = s_ * h * w
        xd, xtd = self.x.to(DEV), self.xt.to(DEV)
        wq, wk, wv, wm = (t.to(DEV) for t in (self.wq, self.wk, self.wv, self.wm))
        norm = self.norm.to(DEV)
        qp, _, _ = o.linear_planes(xd, (wq,))
        kv, _, n2 = o.linear_planes(xtd, (wk, wv))
        res = xd if self.residual else None
        got = {'q_planes': _bf(qp, m, C), 'kv_planes': _bf(kv, m, 2 * C)}
        got['attn'] = o.window_attention_planes((qp, m, C, 0), (kv, m, n2, 0), (kv, m, n2, C), s_, h, w, *geo, self.rot).reshape(m, C)
        got['merge'] = o.window_attention_merge((qp, m, C, 0), (kv, m, n2, 0), (kv, m, n2, C), s_, h, w, *geo, self.rot, wm, norm,
                                                res).reshape(m, C)
        f_, r_, k_ = (ctypes.c_int() for _ in range(3))
        o.lib.um_window_attn_plan(s_, h, w, geo[0], geo[1], ctypes.byref(f_), ctypes.byref(r_), ctypes.byref(k_))
        split = r_.value > 0
        qm, c = _lib_census(o.lib, lambda: o.window_attention_qproj_merge(xd, wq, (kv, m, n2, 0), (kv, m, n2, C), s_, h, w, *geo, self.rot,
                                                                          wm, norm, res))
        assert (c['wattn_ksplit'], c['wattn_tile']) == ((1, 0) if split else (0, 1)), (c, split)
        if self.kind == 'ksplit':
            assert (f_.value, r_.value, k_.value) == (0, 48, 4)                       # all key-split, 4 parts
        got['qproj_merge'] = qm.reshape(m, C)
        return got, (got['q_planes'], got['kv_planes']), f'qproj: wattn_ksplit x{k_.value}' if split else 'qproj: wattn_tile'


ATTN_LAYER_CASES = ([('rotate', (False, True)), ('rotate', (True, False))] + [('prologue', g) for g in PROLOGUE_GEOS] +
                    [('ksplit', (1, 64, 96, 32, 48, 16, 24))])


@pytest.mark.parametrize('kind,case', ATTN_LAYER_CASES)
def test_attention_layer_fast(ops_fast, kind, case):
    """The planes, merge and q-projection + merge variants in bf16 against the emulation (until now compared only with each other):
    bounds for 'attn' and 'merge' / 'qproj_merge' as in the module docstring; the projections' planes 2 U |E64| + 2e-5 max(1, |E64|).
    The q-projection prologue's own q (window_attn.hip:407-409) is not observable; um_linear_fwd's planes of the same product stand in
    for it (same operands, another accumulation order: the exact-mode test ties the two forms to 2e-5)."""
    AttnLayer(kind, case).check(ops_fast, f'layer-{kind}-{"x".join(str(x) for x in case)}')


# ------------------------------------------------------------------------------------------------ global matching / propagation
class Matching(Case):
    """Flow (both directions), stereo and prop_global with 2 and 1 value channels from one pair of token maps.  gsv3 / gsv4 round nothing
    but the operand planes, so the bound is the exact-mode floor alone."""

    def __init__(self, kind, case):
        self.kind = kind
        self.bidir = self.stereo = True
        self.tol = {'flow': 2e-3, 'stereo': 1e-3, 'prop2': 2e-3, 'prop1': 2e-3}        # test_global_matching_random_shapes
        self.expect = None
        if kind == 'shape':
            b, h, w = case
            f0, f1 = rnd(400 + h, b, C, h, w, scale=2.0), rnd(401 + w, b, C, h, w, scale=2.0)
            f1 = 0.6 * f0.roll((1, -2), (2, 3)) + 0.4 * f1
            self.t0, self.t1 = tok(f0), tok(f1)
            self.vals = [rnd(402, b, 2, h, w, scale=3.0)]
            self.expect = {(1, 32, 32): 'gsv3', (36, 24, 40): 'gsv4'}.get(tuple(case))
        elif kind == 'chunks':                       # test_global_matching_chunks_longer_than_a_query_tile
            b, h, w = case
            f0, f1 = rnd(90, b, C, h, w, scale=0.7), rnd(91, b, C, h, w, scale=0.7)
            self.t0, self.t1 = tok(f0), tok(f1)
            self.vals = [rnd(402, b, 2, h, w, scale=3.0)]
            self.tol = {'flow': 1e-3, 'stereo': 1e-3, 'prop2': 2e-3, 'prop1': 2e-3}
            self.expect = 'gsv4'
        else:                                        # test_global_matching_offset_renormalisation
            name, b = case
            h, w = 24, 40
            L = h * w
            f0, f1 = rnd(70, b, L, C), rnd(71, b, L, C)
            if name == 'late_maximum':
                gain = torch.full((L,), 0.3)
                gain[-70:] = 7.0
                f1 = f1 * gain[None, :, None]
            elif name == 'huge_jump':
                f0, f1 = f0 * 6.0, f1 * 0.05
                f1[:, 500:520] = 14.0 * rnd(72, b, 20, C)
            elif name == 'all_negative':
                u = rnd(73, 1, 1, C) * 4.0
                f0, f1 = u + 0.5 * f0, -u + 0.5 * f1
            else:
                f0, f1 = f0 * 0.03, f1 * 0.03
            self.t0, self.t1 = f0.contiguous(), f1.contiguous()
            self.vals = [rnd(402, b, 2, h, w, scale=3.0)]
            self.tol = {'flow': 5e-3, 'stereo': 1e-3, 'prop2': 2e-3, 'prop1': 2e-3}   # flow: that test's own maximum
            self.expect = 'gsv3' if b == 1 else 'gsv4'
        self.h, self.w = h, w
        if self.vals:
            self.vals.append(self.vals[0][:, :1].contiguous())           # one value channel: disparity / depth propagation

    def emulate(self, dtype, rounding, planes=None, want_bound=False, key_mult=None):
        r = em.global_matching(self.t0, self.t1, self.h, self.w, PS, dtype, rounding, values=self.vals, stereo=self.stereo,
                               bidir=self.bidir, key_mult=key_mult)
        out = {'flow': r['flow']}
        if self.stereo:
            out['stereo'] = r['stereo']
        if self.vals:
            out['prop2'], out['prop1'] = r['props']
        return out, {}, None

    def oracle(self):
        b, (h, w) = self.t0.shape[0], (self.h, self.w)
        fm0, fm1 = (t.double().transpose(1, 2).reshape(b, C, h, w) for t in (self.t0, self.t1))
        out = {'flow': hp.global_corr_softmax_flow(fm0, fm1, self.bidir)}
        if self.stereo:
            out['stereo'] = hp.global_corr_softmax_stereo(fm0, fm1)
        if self.vals:
            p = torch.softmax(self.t0.double() @ self.t1.double().transpose(1, 2) / math.sqrt(C), -1)
            for name, v in zip(('prop2', 'prop1'), self.vals):
                out[name] = (p @ v.double().flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, -1, h, w)
        return out

    def floor(self, name, e64):
        return self.tol[name]

    def device(self, o):
        h, w = self.h, self.w
        t0, t1 = self.t0.to(DEV), self.t1.to(DEV)
        assert float(o.lib.um_global_corr_plane_scale(C)) == PS
        got = {}
        got['flow'], c = _lib_census(o.lib, lambda: o.global_corr_softmax_flow(t0, t1, h, w, bidir=self.bidir))
        launches = 2 if self.bidir else 1
        assert c['gsv3'] + c['gsv4'] == launches, c
        which = 'gsv4' if c['gsv4'] else 'gsv3'
        assert c[which] == launches, c
        if self.expect:
            assert which == self.expect, (which, self.expect, c)
        if self.stereo:
            got['stereo'], c = _lib_census(o.lib, lambda: o.global_corr_softmax_stereo(t0, t1, h, w))
            assert c['gsv3'] == 1 and c['gsv4'] == 0, c              # the causal scanline form is gsv3's
        for name, v in zip(('prop2', 'prop1'), self.vals):
            got[name], c = _lib_census(o.lib, lambda: o.prop_global(t0, t1, v.to(DEV), h, w))
            assert c[which] == 1 and c['gsv3'] + c['gsv4'] == 1, (name, c)
        return got, None, which


MATCHING_CASES = ([('shape', s) for s in _random_matching_shapes(26)] + [('shape', (1, 32, 32)), ('shape', (36, 24, 40)),
                  ('chunks', (130, 16, 32))] +
                  [('renorm', (n, b)) for b in (1, 36) for n in ('late_maximum', 'huge_jump', 'all_negative', 'tiny')])


@pytest.mark.parametrize('kind,case', MATCHING_CASES)
def test_global_matching_fast(ops_fast, kind, case):
    """gsv3_kernel / gsv4_kernel<Bf16, 1, NV> and their combine kernels behind flow (both directions), stereo and propagation with two
    and one value channels.  The kernels round nothing after the operand planes (P.V is a chain of fp32 FMAs on fp32 values), so (b)
    is the exact-mode floor of the sibling test: 2e-3 feature cells (flow, propagation; flow 5e-3 for the adversarial orders, 1e-3 for the
    chunk case), 1e-3 stereo.  (1, 32, 32): gsv3 with the two-way key split; (36, 24, 40) and (130, 16, 32): gsv4 (census)."""
    Matching(kind, case).check(ops_fast, f'match-{kind}-{"x".join(str(x) for x in case)}')


# ------------------------------------------------------------------------------------------------ um_linear_fwd
class LinearPlanes(Case):
    rounds = ('planes',)

    def __init__(self, mk):
        self.m, self.n, self.k = mk
        self.a, self.wt = rnd(70, self.m, self.k, scale=2.0), rnd(71, self.n, self.k, scale=0.1)
        self.gelu = self.k == 256

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        e = em.linear(self.a, self.wt, dtype, rounding, gelu=self.gelu)
        return {'planes': e}, ({'planes': em.planes_bound(e)} if want_bound else {}), None

    def oracle(self):
        want = self.a.double() @ self.wt.double().t()
        return {'planes': torch.nn.functional.gelu(want) if self.gelu else want}

    def floor(self, name, e64):
        return 2e-5 * _scale(e64)

    def device(self, o):
        if self.gelu:
            a0, a1 = self.a[:, :128].contiguous(), self.a[:, 128:].contiguous()
            got, _, _ = o.linear_planes(a0.to(DEV), (self.wt.to(DEV),), a1=a1.to(DEV), gelu=True)
        else:
            got, _, _ = o.linear_planes(self.a.to(DEV), tuple(x.contiguous().to(DEV) for x in self.wt.split(128, 0)))
        return {'planes': _bf(got, self.m, self.n)}, None, 'linear'


@pytest.mark.parametrize('mk', [(300, 128, 128), (257, 384, 128), (128, 1024, 256)])
def test_linear_planes_fast(ops_fast, mk):
    """um_linear_fwd<Bf16, 1> writing planes (ragged M, fused q | k | v width, K-concatenated input + GELU): 2 U |E64| + 2e-5 max(1, |E64|)."""
    LinearPlanes(mk).check(ops_fast, f'linear-planes-{"x".join(str(x) for x in mk)}')


class LinearLn(Case):
    """test_linear_layernorm_residual's three forms; nothing is rounded behind the operands: floor only."""

    def __init__(self):
        m = 333
        self.a, self.wt, self.res = rnd(72, m, 128, scale=2.0), rnd(73, 128, 128, scale=0.1), rnd(74, m, 128)
        self.norm, self.ln = _layer_norm(75, 76)
        self.hid, self.w2 = rnd(77, m, 1024), rnd(78, 128, 1024, scale=0.05)

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        out = {'ln': em.linear(self.a, self.wt, dtype, rounding, out='ln', norm=self.ln),
               'ln_res': em.linear(self.a, self.wt, dtype, rounding, out='ln', norm=self.ln, residual=self.res),
               # hid enters as planes written through an identity weight: exactly bf16(hid)
               'ln_planes_in': em.linear(self.hid, self.w2, dtype, rounding, out='ln', norm=self.ln, residual=self.res)}
        return out, {}, None

    def oracle(self):
        g, b, eps = self.ln
        ln = lambda z: torch.nn.functional.layer_norm(z, (128,), g.double(), b.double(), eps)
        w = ln(self.a.double() @ self.wt.double().t())
        return {'ln': w, 'ln_res': w + self.res.double(), 'ln_planes_in': ln(self.hid.double() @ self.w2.double().t()) + self.res.double()}

    def floor(self, name, e64):
        return 5e-5 if name == 'ln_planes_in' else 2e-5

    def device(self, o):
        a, wt, res, norm = self.a.to(DEV), self.wt.to(DEV), self.res.to(DEV), self.norm.to(DEV)
        got = {'ln': o.linear_ln(a, (wt,), norm), 'ln_res': o.linear_ln(a, (wt,), norm, residual=res)}
        hp_, _, _ = o.linear_planes(self.hid.to(DEV), tuple(x.contiguous().to(DEV) for x in torch.eye(1024).split(128, 0)))
        assert torch.equal(_bf(hp_, 333, 1024), em.rb(self.hid))                     # the identity product is exact
        got['ln_planes_in'] = o.linear_ln(hp_, (self.w2.to(DEV),), norm, residual=res, a_planes_k=1024)
        return got, None, 'linear'


def test_linear_layernorm_fast(ops_fast):
    """um_linear_fwd<Bf16, 1> with the LayerNorm epilogue (with / without residual, planes input at K = 1024): no in-kernel
    rounding, so every element within the exact-mode tolerance (2e-5; 5e-5 at K = 1024) of the as-rounded fp64 emulation."""
    LinearLn().check(ops_fast, 'linear-ln-333')


# ------------------------------------------------------------------------------------------------ FFN, FFN + kv4, kv4
class Ffn(Case):
    rounds = ('out',)

    def __init__(self, m, hidden, seed=80):
        self.m, self.hidden = m, hidden
        if seed == 80:                                # test_fused_ffn_kernel
            self.x, self.y = rnd(80, m, 128, scale=1.5), rnd(81, m, 128, scale=1.5)
            self.w1, self.w2 = rnd(82, hidden, 256, scale=0.08), rnd(83, 128, hidden, scale=0.06)
            self.norm, self.ln = _layer_norm(84, 85)
        else:                                         # test_ffn_with_the_next_blocks_kv_projection
            self.x, self.y = rnd(1400, m, 128, scale=1.5), rnd(1401, m, 128, scale=1.5)
            self.w1, self.w2 = rnd(1402, hidden, 256, scale=0.08), rnd(1403, 128, hidden, scale=0.06)
            self.norm, self.ln = _layer_norm(1404, 1405)
            self.ws = tuple(rnd(1410 + i, 128, 128, scale=0.09) for i in range(4))
        self.kv = seed != 80
        if self.kv:
            self.rounds = ('out', 'kv')

    def emulate(self, dtype, rounding, planes=None, want_bound=False, hidden_mult=None):
        r = em.ffn(self.x, self.y, self.w1, self.w2, self.ln, dtype, rounding, hidden_mult=hidden_mult, want_bound=want_bound)
        out, bounds = ({'out': r[0]}, {'out': r[1]}) if want_bound else ({'out': r}, {})
        if self.kv:                                   # the projections of the given (device / E64) FFN output, an fp32 tensor
            src = planes if planes is not None else (out['out'].float() if rounding else out['out'])
            out['kv'] = em.kv4(src, self.ws, dtype, rounding)
            if want_bound:
                bounds['kv'] = em.planes_bound(out['kv'])
            return out, bounds, out['out'].float()
        return out, bounds, None

    def oracle(self):
        g, b, eps = self.ln
        hid = torch.nn.functional.gelu(torch.cat([self.x, self.y], 1).double() @ self.w1.double().t())
        t64 = self.x.double() + torch.nn.functional.layer_norm(hid @ self.w2.double().t(), (128,), g.double(), b.double(), eps)
        out = {'out': t64}
        if self.kv:
            out['kv'] = torch.stack([t64 @ w_.double().t() for w_ in self.ws], 0)
        return out

    def floor(self, name, e64):
        return 3e-5 if name == 'out' else 3e-6 * 40            # test_fused_ffn_kernel; test_kv4_projection's exact-mode maximum

    def device(self, o):
        x, y, w1, w2, norm = self.x.to(DEV), self.y.to(DEV), self.w1.to(DEV), self.w2.to(DEV), self.norm.to(DEV)
        hsplit = o.lib.um_ffn_split_workspace_bytes(self.m, self.hidden) > 0
        if self.kv:
            ws = tuple(w_.to(DEV) for w_ in self.ws)
            (out, kv), c = _lib_census(o.lib, lambda: o.ffn_ln_kv(x, y, w1, w2, norm, ws))
            assert c['ffn_hsplit'] == 1 and c['ffn_tile'] == 0, c                      # m = 1000: the hidden-split path
            got = {'out': out, 'kv': _bf(kv, 4 * self.m, 128).view(4, self.m, 128)}
            return got, out.cpu(), 'ffn_hsplit + kv4'
        out, c = _lib_census(o.lib, lambda: o.ffn_ln(x, y, w1, w2, norm))
        assert (c['ffn_hsplit'], c['ffn_tile']) == ((1, 0) if hsplit else (0, 1)), (c, hsplit)
        return {'out': out}, None, 'ffn_hsplit' if hsplit else 'ffn_tile'


@pytest.mark.parametrize('m,hidden', [(128, 1024), (333, 1024), (1000, 64), (4096 + 17, 512)])
def test_ffn_fast(ops_fast, m, hidden):
    """um_ffn_ws_fwd<Bf16, 1>: gelu(hidden) is packed for the W2 product -> d z_n = 2 U sum_h |g_h| |W2_nh| through the LayerNorm
    bound, + 3e-5 (the exact-mode tolerance)."""
    Ffn(m, hidden).check(ops_fast, f'ffn-{m}x{hidden}')


def test_ffn_kv_fast(ops_fast):
    """um_ffn_kv_fwd<Bf16, 1> at m = 1000 (hidden split + um_kv4_fwd inside the call): the FFN as above; the k | v planes against
    the emulated projections of the DEVICE's FFN output, 2 U |E64| + 1.2e-4."""
    Ffn(1000, 1024, seed=1400).check(ops_fast, 'ffn-kv-1000x1024')


class Kv4(Case):
    rounds = ('kv',)

    def __init__(self, m):
        self.m = m
        self.xs = rnd(1300 + m, m, 128, scale=1.7)
        self.ws = [rnd(1310 + i, 128, 128, scale=0.09) for i in range(4)]

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        e = em.kv4(self.xs, self.ws, dtype, rounding)
        return {'kv': e}, ({'kv': em.planes_bound(e)} if want_bound else {}), None

    def oracle(self):
        return {'kv': torch.stack([self.xs.double() @ w_.double().t() for w_ in self.ws], 0)}

    def floor(self, name, e64):
        return 3e-6 * 40

    def device(self, o):
        kv = o.kv4_planes(self.xs.to(DEV), tuple(w_.to(DEV) for w_ in self.ws))
        return {'kv': _bf(kv, 4 * self.m, 128).view(4, self.m, 128)}, None, 'kv4'


@pytest.mark.parametrize('m', [128, 1000, 2 * 6144 + 40])
def test_kv4_fast(ops_fast, m):
    """um_kv4_fwd<Bf16, 1>: blocked planes [4][M][128], 2 U |E64| + 1.2e-4 (test_kv4_projection's exact-mode maximum)."""
    Kv4(m).check(ops_fast, f'kv4-{m}')


# ------------------------------------------------------------------------------------------------ new in both modes: linear_bias
class LinearBias(Case):
    """um_linear_bias_fwd: fp32 out; planes out with out_mul, bias_mul != 1; planes in (a_planes_k) -> fp32 and -> planes."""
    rounds = ('planes', 'planes2')
    OUT_MUL, BIAS_MUL = PS, 0.75

    def __init__(self, m):
        self.m = m
        self.a, self.wt, self.bias = rnd(1600 + m, m, 128, scale=2.0), rnd(1601, 128, 128, scale=0.1), rnd(1602, 128)
        self.w2, self.b2 = rnd(1603, 128, 128, scale=0.1), rnd(1604, 128)

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        out = {'f32': em.linear(self.a, self.wt, dtype, rounding, bias=self.bias, out='f32'),
               'planes': em.linear(self.a, self.wt, dtype, rounding, bias=self.bias, out_mul=self.OUT_MUL, bias_mul=self.BIAS_MUL)}
        src = planes if (rounding and planes is not None) else out['planes']
        out['f32_planes_in'] = em.linear(src, self.w2, dtype, rounding, bias=self.b2, out='f32', a_is_planes=True)
        out['planes2'] = em.linear(src, self.w2, dtype, rounding, bias=self.b2, out_mul=1.0, bias_mul=self.BIAS_MUL, a_is_planes=True)
        bounds = {k: em.planes_bound(out[k]) for k in ('planes', 'planes2')} if want_bound else {}
        return out, bounds, out['planes']

    def oracle(self):
        a, w_, b = self.a.double(), self.wt.double(), self.bias.double()
        p = (a @ w_.t()) * self.OUT_MUL + b * self.BIAS_MUL
        return {'f32': a @ w_.t() + b, 'planes': p, 'f32_planes_in': p @ self.w2.double().t() + self.b2.double(),
                'planes2': p @ self.w2.double().t() + self.b2.double() * self.BIAS_MUL}

    def floor(self, name, e64):
        return 2e-5 * _scale(e64)                     # the linear kernel's exact-mode tolerance (test_linear_planes_and_gelu)

    def device(self, o):
        a, wt, bias, w2, b2 = (t.to(DEV) for t in (self.a, self.wt, self.bias, self.w2, self.b2))
        m = self.m
        dec = (lambda p, n: _bf(p, m, n)) if o.nplanes == 1 else (lambda p, n: p.view(torch.float16).view(2, m, n).double().sum(0).cpu())
        pl = o.linear_bias(a, wt, bias, out_mul=self.OUT_MUL, bias_mul=self.BIAS_MUL, planes=True)
        got = {'f32': o.linear_bias(a, wt, bias), 'planes': dec(pl, 128),
               'f32_planes_in': o.linear_bias(pl, w2, b2, a_planes_k=128),
               'planes2': dec(o.linear_bias(pl, w2, b2, bias_mul=self.BIAS_MUL, planes=True, a_planes_k=128), 128)}
        return got, got['planes'], 'linear_bias'


@pytest.mark.parametrize('m', [300, 257])
def test_linear_bias_fast(ops_fast, m):
    """um_linear_bias_fwd<Bf16, 1>: out_mul and bias_mul are applied before the pack.  fp32 outputs: floor only (2e-5 max(1, |E64|));
    plane outputs: 2 U |E64| + that floor.  The planes-in launches are compared on the device's own planes."""
    LinearBias(m).check(ops_fast, f'linear-bias-{m}')


@pytest.mark.parametrize('m', [300, 257])
def test_linear_bias_exact(ops, m):
    """The same four launches in exact mode against fp64: 2e-5 max(1, |want|), the linear kernel's tolerance.  The planes-in launches
    read hi + lo planes of the first result (22 bits), so their reference is evaluated on the recombined device planes."""
    case = LinearBias(m)
    got, planes, _ = case.device(ops)
    want = case.oracle()
    p = planes.double()
    want['f32_planes_in'] = p @ case.w2.double().t() + case.b2.double()
    want['planes2'] = p @ case.w2.double().t() + case.b2.double() * case.BIAS_MUL
    for name in sorted(want):
        d = (got[name].double().cpu() - want[name]).abs().max().item()
        assert d < 2e-5 * _scale(want[name]), (name, d)


# ------------------------------------------------------------------------------------------------ new in both modes: projected propagation
PROJ_SHAPES = [(1, 3, 10), (2, 9, 1), (3, 23, 37), (1, 32, 32), (36, 24, 40)]


class PropProjected(Case):
    """HipOps.prop_global_projected: q = Wq x + bq, k = Wk q + bk (planes through um_linear_bias_fwd), softmax(q k^T / sqrt C) value
    with 2 and 1 value channels.  Weights and tokens give logits of about +-40 (checked on the host by the self test)."""
    rounds = ('q_planes', 'k_planes')

    def __init__(self, shape):
        b, h, w = shape
        self.shape = shape
        self.x = rnd(1700 + h, b, h * w, C, scale=1.0)
        self.qw, self.qb = rnd(1701, C, C, scale=0.16), rnd(1702, C, scale=0.3)
        self.kw, self.kb = rnd(1703, C, C, scale=0.16), rnd(1704, C, scale=0.3)
        self.kw = self.kw + 0.3 * torch.eye(C)        # a key that resembles its query: peaked rows as in the trained layer
        v2 = rnd(1705, b, 2, h, w, scale=3.0)
        self.vals = {'prop2': v2, 'prop1': v2[:, :1].contiguous()}

    def logits(self):
        q = self.x.double() @ self.qw.double().t() + self.qb.double()
        k = q @ self.kw.double().t() + self.kb.double()
        return torch.bmm(q, k.transpose(1, 2)) / math.sqrt(C)

    def emulate(self, dtype, rounding, planes=None, want_bound=False):
        b, h, w = self.shape
        out, qk = {}, None
        use = planes if rounding else None
        for name, v in self.vals.items():
            out[name], qk = em.prop_projected(self.x, self.qw, self.qb, self.kw, self.kb, v, h, w, PS, dtype, rounding, planes=use)
        if rounding:                                  # the projection stages themselves (k from the given q planes)
            q = em.linear(self.x.reshape(-1, C), self.qw, dtype, rounding, bias=self.qb, out_mul=PS, bias_mul=PS)
            src = q if use is None else use[0]
            k = em.linear(src, self.kw, dtype, rounding, bias=self.kb, out_mul=1.0, bias_mul=PS, a_is_planes=True)
        else:
            q, k = qk[0] * PS, qk[1] * PS
        out['q_planes'], out['k_planes'] = q, k
        bounds = {n: em.planes_bound(out[n]) for n in ('q_planes', 'k_planes')} if want_bound else {}
        return out, bounds, (q, k)

    def oracle(self):
        b, h, w = self.shape
        q = self.x.double() @ self.qw.double().t() + self.qb.double()
        k = q @ self.kw.double().t() + self.kb.double()
        p = torch.softmax(torch.bmm(q, k.transpose(1, 2)) / math.sqrt(C), -1)
        out = {n: (p @ v.double().flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, -1, h, w) for n, v in self.vals.items()}
        out['q_planes'], out['k_planes'] = (q * PS).reshape(-1, C), (k * PS).reshape(-1, C)
        return out

    def floor(self, name, e64):
        return 2e-5 * _scale(e64) if name.endswith('planes') else 2e-3

    def modules(self):
        qp, kp = torch.nn.Linear(C, C), torch.nn.Linear(C, C)
        with torch.no_grad():
            qp.weight.copy_(self.qw), qp.bias.copy_(self.qb), kp.weight.copy_(self.kw), kp.bias.copy_(self.kb)
        return qp.to(DEV), kp.to(DEV)

    def device(self, o):
        b, h, w = self.shape
        qm, km = self.modules()
        xd = self.x.to(DEV)
        assert float(o.lib.um_global_corr_plane_scale(C)) == PS
        got, which = {}, None
        for name, v in self.vals.items():
            got[name], c = _lib_census(o.lib, lambda: o.prop_global_projected(xd, qm, km, v.to(DEV), h, w))
            assert c['gsv3'] + c['gsv4'] == 1, c
            which = 'gsv4' if c['gsv4'] else 'gsv3'
        expect = {(1, 32, 32): 'gsv3', (36, 24, 40): 'gsv4'}.get(tuple(self.shape))
        assert expect is None or which == expect, (which, expect)
        if o.nplanes != 1:
            return got, None, which
        # the two projection launches as prop_global_projected issues them: the planes its attention launch reads
        qp = o.linear_bias(xd.reshape(b * h * w, C), qm.weight, qm.bias, out_mul=PS, bias_mul=PS, planes=True)
        kp = o.linear_bias(qp, km.weight, km.bias, out_mul=1.0, bias_mul=PS, planes=True, a_planes_k=C)
        got['q_planes'], got['k_planes'] = _bf(qp, b * h * w, C), _bf(kp, b * h * w, C)
        return got, (got['q_planes'], got['k_planes']), which


@pytest.mark.parametrize('shape', PROJ_SHAPES)
def test_prop_global_projected_fast(ops_fast, shape):
    """um_linear_bias_fwd (planes) x 2 + um_prop_global_attn_planes<Bf16, 1> with 2 and 1 value channels.  The attention stage is
    compared on the device's own q / k planes and rounds nothing: floor 2e-3 (the exact-mode propagation tolerance); the planes
    2 U |E64| + 2e-5 max(1, |E64|)."""
    PropProjected(shape).check(ops_fast, f'prop-projected-{"x".join(str(x) for x in shape)}')


@pytest.mark.parametrize('shape', PROJ_SHAPES)
def test_prop_global_projected_exact(ops, shape):
    """Exact mode against fp64 of q = Wq x + bq, k = Wk q + bk, softmax(q k^T / sqrt C) value: max < 2e-3 and mean < 1e-4, the
    tolerances of test_global_matching_random_shapes."""
    case = PropProjected(shape)
    got, _, _ = case.device(ops)
    want = case.oracle()
    for name in ('prop2', 'prop1'):
        d = (got[name].double().cpu() - want[name]).abs()
        assert torch.isfinite(got[name]).all() and d.max().item() < 2e-3 and d.mean().item() < 1e-4, (shape, name, d.max().item(), d.mean().item())


@pytest.mark.parametrize('shape', PROJ_SHAPES[2:])
def test_prop_global_one_value_channel_exact(ops, shape):
    """um_prop_global_attn with ONE value channel (launch_gsv<1, false>: (2 + 1)-float partial rows in both combine kernels) in exact
    mode at a ragged shape, the gsv3 key split and gsv4's mid-tile chunks: max < 2e-3, mean < 1e-4."""
    case = Matching('shape', shape)
    want = case.oracle()['prop1']
    got, c = _lib_census(ops.lib, lambda: ops.prop_global(case.t0.to(DEV), case.t1.to(DEV), case.vals[1].to(DEV), case.h, case.w))
    expect = {(1, 32, 32): 'gsv3', (36, 24, 40): 'gsv4'}.get(tuple(shape))
    assert expect is None or c[expect] == 1, c
    d = (got.double().cpu() - want).abs()
    assert torch.isfinite(got).all() and d.max().item() < 2e-3 and d.mean().item() < 1e-4, (shape, d.max().item(), d.mean().item())
