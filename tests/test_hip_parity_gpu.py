"""GPU parity tests: every HIP entry point (called through the C ABI via ctypes) against the CPU oracle
evaluated in float64, on the committed golden inputs plus seeded larger / ragged shapes, and end to end.

Tolerances (written where used):
  exact mode (fp16 hi+lo split operands, fp32 accumulate): the kernels must match an fp64 evaluation as
  closely as the fp32 reference itself does -> abs 5e-5 on O(1) attention outputs, 2e-3 feature cells on
  expected coordinates with +-100 logits.
  fast mode (bf16 operands): 3e-2 relative to the output scale.
"""
import math

import pytest
import torch

from oracle import hotpath as hp
from oracle import model as om
from tests.dispatch_boundaries import merged_layer_reference
from unimatch_amd import UniMatch
from unimatch_amd.ops import HipOps
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
C = 128
DEV = 'cuda'


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tok(fmap):
    return fmap.flatten(2).transpose(1, 2).contiguous()


def err(a, b):
    d = (a.double().cpu() - b.double().cpu()).abs()
    return d.max().item(), d.mean().item()


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


@pytest.fixture(scope='module')
def ops_fast():
    return HipOps('fast')


# ------------------------------------------------------------------ attention
def _geom(tag, h, w, k, shift):
    if tag.startswith('win2d'):
        return (h // k, w // k, (h // k // 2) if shift else 0, (w // k // 2) if shift else 0)
    if tag.startswith('winrow'):
        return (1, w // k, 0, (w // k // 2) if shift else 0)
    if tag.startswith('row'):
        return (1, w, 0, 0)
    return (h, w, 0, 0)


def test_window_attention_golden_cases(ops, ops_fast, golden):
    g = golden('attention')
    for tag in sorted({k.split('.')[0] for k in g.keys()}):
        h, w, k, shift = (int(x) for x in g[f'{tag}.meta'])
        geom = _geom(tag, h, w, k, shift)
        q, kk, v = g[f'{tag}.q'], g[f'{tag}.k'], g[f'{tag}.v']
        want = hp.window_attention(q.double(), kk.double(), v.double(), h, w, *geom)
        got = ops.window_attention(q.to(DEV), kk.to(DEV), v.to(DEV), h, w, *geom)
        mx, mean = err(got, want)
        assert mx < 5e-5 * max(1.0, want.abs().max().item()), (tag, mx, mean)
        # the fp32 reference output stored in the fixture is just as close
        assert err(got, g[f'{tag}.out'])[0] < 1e-4 * max(1.0, want.abs().max().item()), tag
        got_f = ops_fast.window_attention(q.to(DEV), kk.to(DEV), v.to(DEV), h, w, *geom)
        assert err(got_f, want)[1] < 3e-2 * want.abs().mean().item() + 1e-3, (tag, 'fast')


@pytest.mark.parametrize('case', [
    # streams, h, w, win_h, win_w, shift_h, shift_w, scale
    (2, 16, 24, 8, 12, 4, 6, 1.0),        # 96-token windows: ragged 128-query tile, 2 key tiles
    (1, 20, 28, 10, 14, 5, 7, 2.0),       # 140-token windows: 2 query tiles, ragged key tile
    (2, 32, 48, 16, 24, 8, 12, 1.5),      # 384-token windows (config-4 scale-1 window size)
    (1, 24, 40, 24, 40, 0, 0, 1.0),       # one full window of 960 tokens
    (2, 6, 60, 1, 30, 0, 15, 2.0),        # config-3 style 1-D shifted windows of 30
    (2, 5, 120, 1, 120, 0, 0, 1.0),       # full scanlines of 120
])
def test_window_attention_larger_shapes(ops, case):
    s, h, w, wh, ww, sh, sw, scale = case
    q, k, v = (rnd(10 + i, s, h * w, C, scale=scale) for i in range(3))
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
    got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
    mx, mean = err(got, want)
    assert mx < 5e-5 * max(1.0, want.abs().max().item()), (case, mx, mean)


def _random_window_geometries(count, seed=2024):
    """Deterministic pseudo-random (streams, h, w, win_h, win_w, shift_h, shift_w): window sizes that are not multiples of the
    32-key / 128-query tiles, 1-row and 1-column windows, arbitrary shifts below the window size (the kernel takes any; the
    reference only ever uses win // 2), maps of 1 .. 4 windows per axis."""
    import random
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        win_h, win_w = rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 12]), rng.choice([1, 3, 5, 8, 13, 17, 24, 30, 33, 40])
        nwy, nwx = rng.choice([1, 2, 2, 3, 4]), rng.choice([1, 2, 2, 3, 4])
        h, w = win_h * nwy, win_w * nwx
        if h * w > 4000 or win_h * win_w > 700:
            continue
        sh = rng.randrange(0, win_h) if nwy > 1 and win_h > 1 and rng.random() < 0.7 else 0
        sw = rng.randrange(0, win_w) if nwx > 1 and win_w > 1 and rng.random() < 0.7 else 0
        out.append((rng.choice([1, 2, 3]), h, w, win_h, win_w, sh, sw))
    return out


@pytest.mark.parametrize('geo', _random_window_geometries(28))
def test_window_attention_random_geometries(ops, geo):
    """um_window_attn_fwd against the fp64 oracle over pseudo-random window geometries (see the generator)."""
    s_, h, w, wh, ww, sh, sw = geo
    q, k, v = (rnd(700 + i + h * w, s_, h * w, C, scale=1.5) for i in range(3))
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
    got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
    assert torch.isfinite(got).all(), geo
    mx, mean = err(got, want)
    assert mx < 5e-5 * max(1.0, want.abs().max().item()), (geo, mx, mean)


def test_window_attention_forced_rescale_and_mask_dominance(ops):
    """A spiked key far down the window forces the running max to jump late (every earlier tile must be
    rescaled exactly once), and a masked key whose logit beats the own region by more than 100 must WIN the
    softmax (the reference adds -100, it does not exclude)."""
    s, h, w, wh, ww = 1, 16, 24, 8, 12
    q, k, v = (rnd(20 + i, s, h * w, C) for i in range(3))
    k[0, 200] = q[0, 10] * 6.0                 # token 200 strongly matches token 10's query direction
    for (sh, sw) in ((0, 0), (4, 6)):
        want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
        got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
        assert err(got, want)[0] < 1e-4 * max(1.0, want.abs().max().item())
    # mask dominance: last window of the shifted map mixes regions; make one cross-region logit huge
    q2, k2, v2 = (rnd(30 + i, s, h * w, C) for i in range(3))
    idx, label = hp.window_index(h, w, wh, ww, 4, 6)
    win = idx.shape[0] - 1
    a = int(idx[win, 0])
    other = [int(idx[win, j]) for j in range(idx.shape[1]) if label[win, j] != label[win, 0]]
    assert other
    q2[0, a] = 0.0
    q2[0, a, 0] = 60.0
    k2[0, :, 0] = 0.0
    k2[0, other[0], 0] = 60.0                   # raw logit 3600/sqrt(128) = 318 > 100 above everything else
    want = hp.window_attention(q2.double(), k2.double(), v2.double(), h, w, wh, ww, 4, 6)
    got = ops.window_attention(q2.to(DEV), k2.to(DEV), v2.to(DEV), h, w, wh, ww, 4, 6)
    assert (want[0, a] - v2[0, other[0]].double()).abs().max() < 1e-6      # the masked key dominates
    assert err(got, want)[0] < 1e-4 * max(1.0, want.abs().max().item())


def _census(fn):
    """Run fn() with the key-tile census on; returns (result, counters)."""
    from unimatch_amd import _abi
    _abi.attn_tile_census(True)
    try:
        out = fn()
    finally:
        counts = _abi.attn_tile_census(False)
    return out, counts


def test_window_attention_masked_tile_skip_margin_and_fallback(ops, ops_fast):
    """Round 6: wholly masked (query workgroup, key tile) pairs are probed and dropped only under a bound.  Geometry with
    class-uniform tiles (64x32 map, 2x2 windows of 32x16 = 512 tokens, shift 16/8: class sizes 512 | 256+256 | 256+256 | 4 x 128).
    (a) random data: every masked tile is dropped, the census is the closed form, the result is the oracle's;
    (b) one masked key whose logit sits 41 below the row maximum (-100 included): still dropped; 39 below: the tile is computed;
    (c) a masked key that must WIN the softmax (logit 318 - 100 above everything): the fallback computes it and it dominates;
    (d) one class of keys scaled by 12: many probes fail, result still the oracle's."""
    s, h, w, wh, ww, sh, sw = 2, 64, 32, 32, 16, 16, 8
    n, tiles = wh * ww, wh * ww // 32
    q, k, v = (rnd(50 + i, s, h * w, C) for i in range(3))
    idx, label = hp.window_index(h, w, wh, ww, sh, sw)

    def run(o, q_, k_, v_):
        want = hp.window_attention(q_.double(), k_.double(), v_.double(), h, w, wh, ww, sh, sw)
        got, counts = _census(lambda: o.window_attention(q_.to(DEV), k_.to(DEV), v_.to(DEV), h, w, wh, ww, sh, sw))
        return want, got, counts

    # closed form of the census: per stream 4 windows x 4 workgroups; masked tiles per workgroup 0 / 8 / 8 / 12 of 16
    probed_all = s * 4 * (0 + 8 + 8 + 12)
    full_all = s * 4 * (16 + 8 + 8 + 4)
    for o, tol in ((ops, 5e-5), (ops_fast, None)):
        want, got, c = run(o, q, k, v)
        assert c == {'full': full_all, 'probed': probed_all, 'probed_then_computed': 0, 'workgroups': s * 16}, c
        if tol:
            assert err(got, want)[0] < tol * max(1.0, want.abs().max().item())
        else:
            assert err(got, want)[1] < 3e-2 * want.abs().mean().item() + 1e-3
    # (b) margins 41 and 39 around the threshold of 40: query a of the corner window, own-class logits exactly 0 (channel 0 of every
    # key is 0, the query is e0 * x), ONE key of another class with logit x*y/sqrt(C) - 100 = -40 -/+ 1
    win = idx.shape[0] - 1
    a = int(idx[win, 0])
    other = [int(idx[win, j]) for j in range(n) if label[win, j] != label[win, 0]]
    for delta, expect_computed in ((-1.0, 0), (+1.0, 1)):
        q2, k2 = q.clone(), k.clone()
        x = math.sqrt((60.0 + delta) * math.sqrt(C))
        q2[0, a] = 0.0
        q2[0, a, 0] = x
        k2[:, :, 0] = 0.0
        k2[0, other[5], 0] = x
        want, got, c = run(ops, q2, k2, v)
        assert c['probed'] == probed_all and c['probed_then_computed'] == expect_computed, (delta, c)
        assert c['full'] == full_all + expect_computed
        assert err(got, want)[0] < 5e-5 * max(1.0, want.abs().max().item())
    # (c) mask dominance through the fallback
    q2, k2 = q.clone(), k.clone()
    q2[0, a] = 0.0
    q2[0, a, 0] = 60.0
    k2[:, :, 0] = 0.0
    k2[0, other[-1], 0] = 60.0
    for o in (ops, ops_fast):
        want, got, c = run(o, q2, k2, v)
        assert c['probed_then_computed'] == 1, c
        assert (want[0, a] - v[0, other[-1]].double()).abs().max() < 1e-6
        assert (got[0, a].cpu().double() - v[0, other[-1]].double()).abs().max() < (1e-4 if o is ops else 3e-2)
        if o is ops:
            assert err(got, want)[0] < 1e-4 * max(1.0, want.abs().max().item())
    # (d) a whole class of loud keys: the keys of the wrapped columns x 12 -> logits of std 12, maxima ~ 40-45 above the quiet own
    # class; shifted so that the threshold of 60 cuts through the distribution
    k3 = k.clone()
    wrapped = torch.zeros(h * w, dtype=torch.bool)
    wrapped[idx[label % 3 == 2]] = True                  # column band 2 of unimatch/utils.py:95-100
    k3[:, wrapped] *= 16.0
    want, got, c = run(ops, q, k3, v)
    assert 0 < c['probed_then_computed'] < c['probed'], c
    assert err(got, want)[0] < 5e-5 * max(1.0, want.abs().max().item())


def test_window_attention_tile_census_at_config2_size(ops):
    """At BASELINE config 2's layer geometry (64x96, 2x2 windows of 1536 tokens, shift 16/24) the shifted launch computes 56.25 % of
    its key tiles and probes the rest; the unshifted one computes all; both equal the fp64 oracle on one stream."""
    s, h, w, wh, ww = 2, 64, 96, 32, 48
    q, k, v = rnd(60, s, h * w, C, scale=1.5), rnd(61, s, h * w, C, scale=1.5), rnd(62, s, h * w, C)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    got0, c0 = _census(lambda: ops.window_attention(qd, kd, vd, h, w, wh, ww, 0, 0))
    assert c0 == {'full': s * 4 * 12 * 48, 'probed': 0, 'probed_then_computed': 0, 'workgroups': s * 48}, c0
    got1, c1 = _census(lambda: ops.window_attention(qd, kd, vd, h, w, wh, ww, 16, 24))
    assert c1 == {'full': s * 12 * (48 + 24 + 24 + 12), 'probed': s * 12 * (24 + 24 + 36), 'probed_then_computed': 0,
                  'workgroups': s * 48}, c1
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, 16, 24)
    assert err(got1, want)[0] < 5e-5 * max(1.0, want.abs().max().item())


def test_window_attention_properties_at_config2_size(ops, ops_fast):
    """Size-independent properties at BASELINE config 2's layer size (2B=4 here to bound memory): 64x96 map,
    2x2 windows of 1536 tokens.  (a) constant v -> same constant; (b) k = 0 -> plain window mean of v,
    including through the cyclic shift; (c) linearity in v."""
    s, h, w, wh, ww = 4, 64, 96, 32, 48
    q = rnd(40, s, h * w, C, scale=2.0).to(DEV)
    k = rnd(41, s, h * w, C, scale=2.0).to(DEV)
    v = rnd(42, s, h * w, C).to(DEV)
    for o in (ops, ops_fast):
        tol = 1e-5 if o is ops else 2e-2
        for (sh, sw) in ((0, 0), (16, 24)):
            const = torch.full_like(v, 0.75)
            assert (o.window_attention(q, k, const, h, w, wh, ww, sh, sw) - 0.75).abs().max().item() < tol
    out0 = ops.window_attention(q, torch.zeros_like(k), v, h, w, wh, ww, 0, 0)
    vm = v.view(s, 2, wh, 2, ww, C).mean(dim=(2, 4), keepdim=True).expand(s, 2, wh, 2, ww, C).reshape(s, h * w, C)
    assert (out0 - vm).abs().max().item() < 2e-6
    v2 = rnd(43, s, h * w, C).to(DEV)
    a = ops.window_attention(q, k, v, h, w, wh, ww, 16, 24)
    b = ops.window_attention(q, k, v2, h, w, wh, ww, 16, 24)
    ab = ops.window_attention(q, k, 0.5 * v - 2.0 * v2, h, w, wh, ww, 16, 24)
    assert (ab - (0.5 * a - 2.0 * b)).abs().max().item() < 2e-5


def test_window_attention_config2_size_vs_fp64(ops, ops_fast):
    """The attention core at BASELINE config 2's layer geometry (64x96 map, 2x2 windows of 1536 tokens, cyclic shift 16/24 with
    the -100 masks; 2 streams to bound the CPU time) against the fp64 oracle: exact mode within 2x of what fp32 arithmetic
    gives, bf16 mode in its ballpark (full-size kernel-vs-oracle comparisons, not only properties)."""
    s, h, w, wh, ww = 2, 64, 96, 32, 48
    q, k, v = rnd(44, s, h * w, C, scale=1.5), rnd(45, s, h * w, C, scale=1.5), rnd(46, s, h * w, C)
    for (sh, sw) in ((0, 0), (16, 24)):
        want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
        f32 = hp.window_attention(q, k, v, h, w, wh, ww, sh, sw)
        got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
        e_gpu, e_f32 = err(got, want), err(f32, want)
        assert e_gpu[1] <= 2.0 * e_f32[1] + 1e-6 and e_gpu[0] <= 2.0 * e_f32[0] + 1e-7, ((sh, sw), e_gpu, e_f32)
        fast = ops_fast.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
        assert err(fast, want)[1] < 3e-2 * want.abs().max().item() + 1e-3


# ------------------------------------------------------------------ global matching / propagation
@pytest.mark.parametrize('tag', ['soft', 'peaky'])
def test_global_matching_golden(ops, ops_fast, golden, tag):
    g = golden('matching')
    f0, f1 = g[f'{tag}.f0'], g[f'{tag}.f1']
    b, _, h, w = f0.shape
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), True)
    got = ops.global_corr_softmax_flow(t0, t1, h, w, bidir=True)
    assert got.shape == (2 * b, 2, h, w)
    assert err(got, want)[0] < 2e-4, tag                         # feature cells
    assert err(got, g[f'{tag}.global_flow_bidir'])[0] < 5e-4
    assert err(ops.global_corr_softmax_flow(t0, t1, h, w), want[:b])[0] < 2e-4
    want_s = hp.global_corr_softmax_stereo(f0.double(), f1.double())
    got_s = ops.global_corr_softmax_stereo(t0, t1, h, w)
    assert got_s.shape == (b, 1, h, w) and err(got_s, want_s)[0] < 1e-4
    if tag == 'soft':
        assert err(ops_fast.global_corr_softmax_flow(t0, t1, h, w), want[:b])[1] < 5e-2


def test_global_matching_realistic_logits(ops):
    """Feature statistics of the real random-init model (|f| ~ 4: logits reach +-150, very peaky softmax) at
    a ragged size (L = 40*56 = 2240, not a multiple of 64 or 128)."""
    b, h, w = 2, 40, 56
    f0, f1 = rnd(50, b, C, h, w, scale=4.0), rnd(51, b, C, h, w, scale=4.0)
    f1 = 0.7 * f0.roll((3, -5), (2, 3)) + 0.3 * f1               # real correspondences
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), False)
    got = ops.global_corr_softmax_flow(tok(f0).to(DEV), tok(f1).to(DEV), h, w)
    mx, mean = err(got, want)
    assert mean < 2e-4 and mx < 5e-3, (mx, mean)


def test_global_matching_full_size_vs_fp64(ops, ops_fast):
    """BASELINE config-2 size (64 x 96 map, L = 6144: 96 key tiles, split-KV launch) against the fp64 oracle -- the L x L
    fp64 probabilities are 302 MB on the host.  Realistic random-init statistics: |f| ~ 4, logits beyond +-150."""
    b, h, w = 1, 64, 96
    f0, f1 = rnd(60, b, C, h, w, scale=4.0), rnd(61, b, C, h, w, scale=4.0)
    f1 = 0.7 * f0.roll((2, -7), (2, 3)) + 0.3 * f1
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), True)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    got = ops.global_corr_softmax_flow(t0, t1, h, w, bidir=True)
    mx, mean = err(got, want)
    assert mean < 2e-4 and mx < 5e-3, (mx, mean)                   # feature cells
    val = rnd(62, b, 2, h, w, scale=5.0)
    got_p = ops.prop_global(t0, t1, val.to(DEV), h, w)              # q = f0 tokens, k = f1 tokens, values = val
    p = torch.softmax(tok(f0).double() @ tok(f1).double().transpose(1, 2) / math.sqrt(C), -1)
    want_p = (p @ val.double().flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, 2, h, w)
    mx, mean = err(got_p, want_p)
    assert mean < 2e-4 and mx < 5e-3, (mx, mean)
    fast = ops_fast.global_corr_softmax_flow(t0, t1, h, w)
    assert torch.isfinite(fast).all() and err(fast, want[:b])[1] < 0.5      # bf16 operands on +-150 logits: ballpark only


def _random_matching_shapes(count, seed=77):
    """(batch, h, w): maps whose token count is below one tile, not a multiple of 32 / 64 / 256 (ragged key and query tiles:
    gsv_kernel and the split-KV launch), multiples of 64 at and above 512 tokens with few and with many samples
    (gsv3_kernel / the stream-K gsv4_kernel), one-row and one-column maps."""
    import random
    rng = random.Random(seed)
    out = [(1, 1, 7), (2, 9, 1), (1, 3, 10), (40, 16, 32), (3, 32, 48), (20, 24, 32)]
    while len(out) < count:
        h, w = rng.randrange(2, 41), rng.randrange(2, 61)
        if h * w <= 2600:
            out.append((rng.choice([1, 1, 2, 3, 5]), h, w))
    return out


@pytest.mark.parametrize('shape', _random_matching_shapes(26))
def test_global_matching_random_shapes(ops, shape):
    """um_global_corr_softmax_flow (one direction and both), the stereo form and um_prop_global_attn against the fp64 oracle
    over pseudo-random map sizes (see the generator); features with real correspondences, logits to about +-40."""
    b, h, w = shape
    f0, f1 = rnd(400 + h, b, C, h, w, scale=2.0), rnd(401 + w, b, C, h, w, scale=2.0)
    f1 = 0.6 * f0.roll((1, -2), (2, 3)) + 0.4 * f1
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), True)
    got = ops.global_corr_softmax_flow(t0, t1, h, w, bidir=True)
    assert torch.isfinite(got).all(), shape
    mx, mean = err(got, want)
    assert mean < 1e-4 and mx < 2e-3, (shape, mx, mean)
    assert err(ops.global_corr_softmax_flow(t0, t1, h, w), want[:b])[0] < 2e-3, shape
    got_s = ops.global_corr_softmax_stereo(t0, t1, h, w)
    assert err(got_s, hp.global_corr_softmax_stereo(f0.double(), f1.double()))[0] < 1e-3, shape
    val = rnd(402, b, 2, h, w, scale=3.0)
    p = torch.softmax(tok(f0).double() @ tok(f1).double().transpose(1, 2) / math.sqrt(C), -1)
    want_p = (p @ val.double().flatten(2).transpose(1, 2)).transpose(1, 2).reshape(b, 2, h, w)
    assert err(ops.prop_global(t0, t1, val.to(DEV), h, w), want_p)[0] < 2e-3, shape


@pytest.mark.parametrize('b', [1, 36])           # 1 sample: gsv3_kernel (small launch); 36: gsv4_kernel (>= 8 key tiles per CU)
@pytest.mark.parametrize('case', ['late_maximum', 'huge_jump', 'all_negative', 'tiny'])
def test_global_matching_offset_renormalisation(ops, ops_fast, case, b):
    """The running softmax offset is renormalised lazily (only when a tile's maximum exceeds it by 2^40, on a separate
    path).  Adversarial key orders: the maximum arrives in the last tiles after hundreds of small scores; one jump of more
    than 2^127 (would overflow exp2 if the lazy path were taken); all logits far below zero (the first tile must set a
    NEGATIVE-score offset or everything underflows); logits ~1e-3 (a flat softmax: every key matters)."""
    h, w = 24, 40                                                  # L = 960 = 15 key tiles
    L = h * w
    f0, f1 = rnd(70, b, L, C), rnd(71, b, L, C)
    if case == 'late_maximum':
        gain = torch.full((L,), 0.3)
        gain[-70:] = 7.0                                           # the last two tiles dominate by ~2^60
        f1 = f1 * gain[None, :, None]
    elif case == 'huge_jump':
        f0, f1 = f0 * 6.0, f1 * 0.05
        f1[:, 500:520] = 14.0 * rnd(72, b, 20, C)                  # logits jump from ~+-3 to several hundred
    elif case == 'all_negative':
        u = rnd(73, 1, 1, C) * 4.0
        f0, f1 = u + 0.5 * f0, -u + 0.5 * f1                       # q . k ~ -|u|^2 = about -2000 -> logits ~ -180
    else:
        f0, f1 = f0 * 0.03, f1 * 0.03
    fm0 = f0.transpose(1, 2).reshape(b, C, h, w)
    fm1 = f1.transpose(1, 2).reshape(b, C, h, w)
    want = hp.global_corr_softmax_flow(fm0.double(), fm1.double(), False)
    got = ops.global_corr_softmax_flow(f0.contiguous().to(DEV), f1.contiguous().to(DEV), h, w)
    assert torch.isfinite(got).all(), case
    mx, mean = err(got, want)
    assert mean < 2e-4 and mx < 5e-3, (case, mx, mean)
    # bf16 mode (P.V on the matrix pipe, offset shared by a query's two half-waves): same renormalisation paths; the reference
    # here is the fp64 evaluation of the features ROUNDED AS THE PLANES ARE, so that what is compared is the kernel (bf16
    # probabilities: 2^-9 relative), not the operand rounding
    ps = float(ops_fast.lib.um_global_corr_plane_scale(C))            # the planes carry this factor BEFORE the bf16 rounding
    r0, r1 = (fm0 * ps).bfloat16().double() / ps, (fm1 * ps).bfloat16().double() / ps
    want_f = hp.global_corr_softmax_flow(r0, r1, False)
    got_f = ops_fast.global_corr_softmax_flow(f0.contiguous().to(DEV), f1.contiguous().to(DEV), h, w)
    assert torch.isfinite(got_f).all(), (case, 'fast')
    mx, mean = err(got_f, want_f)
    assert mean < 0.25, (case, 'fast', mx, mean)


def test_global_matching_chunks_longer_than_a_query_tile(ops):
    """gsv4's stream-K decomposition with MORE (batch x query tile) rows than CUs: a workgroup's chunk is then longer than one
    query tile's key range and not a multiple of it, so chunks start and end in mid-tile and carry up to three segments
    (tail of one query tile, a whole one, head of the next).  130 samples of 16 x 32 tokens: 2080 units, chunks of 9 > KT = 8."""
    b, h, w = 130, 16, 32
    f0, f1 = rnd(90, b, C, h, w, scale=0.7), rnd(91, b, C, h, w, scale=0.7)
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), False)
    got = ops.global_corr_softmax_flow(tok(f0).to(DEV), tok(f1).to(DEV), h, w)
    mx, mean = err(got, want)
    assert mean < 2e-5 and mx < 1e-3, (mx, mean)


@pytest.mark.parametrize('scale', [0.1, 1.0, 10.0, 100.0])
def test_exact_mode_operand_scale_sweep(ops, scale):
    """Exact mode splits operands into fp16 hi + lo planes (22 significant bits while the lo plane stays in fp16's normal
    range): full accuracy for element magnitudes in about [2^-3, 2^15]; below that the absolute error floor is ~2^-25, above
    65504 the hi plane saturates (include/unimatch_hip.h, "Operand range").  Inside that documented range -- three decades
    around the O(1)..O(10) activations the model produces -- every kernel must stay within 2x of what fp32 arithmetic gives
    against fp64."""
    b, h, w = 1, 16, 24
    L = h * w
    # --- attention: q, k scaled so that the logits stay O(1..10) (softmax well conditioned), v carries the magnitude
    q, k = rnd(80, 2 * b, L, C), rnd(81, 2 * b, L, C)
    v = rnd(82, 2 * b, L, C) * scale
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, h // 2, w // 2, 0, 0)
    f32 = hp.window_attention(q, k, v, h, w, h // 2, w // 2, 0, 0)
    got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, h // 2, w // 2, 0, 0)
    e_gpu, e_f32 = err(got, want)[1], err(f32, want)[1]
    assert torch.isfinite(got).all() and e_gpu <= 2.0 * e_f32 + 1e-7 * scale, ('attn v', scale, e_gpu, e_f32)
    # --- attention with the magnitude on q and k (logits scale^2-ish): sqrt(scale) each, bounded to a sane logit range
    s2 = min(max(scale, 1e-3), 30.0) ** 0.5
    want = hp.window_attention((q * s2).double(), (k * s2).double(), v.double() / scale, h, w, h // 2, w // 2, 0, 0)
    f32 = hp.window_attention(q * s2, k * s2, v / scale, h, w, h // 2, w // 2, 0, 0)
    got = ops.window_attention((q * s2).to(DEV), (k * s2).to(DEV), (v / scale).to(DEV), h, w, h // 2, w // 2, 0, 0)
    e_gpu, e_f32 = err(got, want)[1], err(f32, want)[1]
    assert torch.isfinite(got).all() and e_gpu <= 2.0 * e_f32 + 2e-7, ('attn qk', scale, e_gpu, e_f32)
    # --- global correlation: features scaled by s2 on both sides
    f0, f1 = rnd(83, b, C, h, w) * s2, rnd(84, b, C, h, w) * s2
    want = hp.global_corr_softmax_flow(f0.double(), f1.double(), False)
    f32 = hp.global_corr_softmax_flow(f0, f1, False)
    got = ops.global_corr_softmax_flow(tok(f0).to(DEV), tok(f1).to(DEV), h, w)
    e_gpu, e_f32 = err(got, want)[1], err(f32, want)[1]
    assert torch.isfinite(got).all() and e_gpu <= 2.0 * e_f32 + 2e-6, ('gsv', scale, e_gpu, e_f32)
    # --- convolution (3x3, 64 -> 64): activations carry the magnitude
    x = rnd(85, 1, 64, 16, 32) * scale
    wt = rnd(86, 64, 64, 3, 3) * 0.05
    want = torch.nn.functional.conv2d(x.double(), wt.double(), None, padding=1)
    f32 = torch.nn.functional.conv2d(x, wt, None, padding=1)
    planes, _ = ops.nchw_to_nhwc(x.to(DEV), want_planes=True, want_f32=False)
    got, _, _ = ops.conv2d_nhwc((planes, 1, 16, 32, 64), wt.to(DEV), None, 1, (1, 1))
    got = got.reshape(1, 16, 32, 64).permute(0, 3, 1, 2)
    e_gpu, e_f32 = err(got, want)[1], err(f32, want)[1]
    assert torch.isfinite(got).all() and e_gpu <= 2.0 * e_f32 + 1e-7 * scale, ('conv', scale, e_gpu, e_f32)


def test_propagation_golden(ops, golden):
    g = golden('propagation')
    proto = UniMatch().feature_flow_attn
    sd = synth_state_dict({k: v.shape for k, v in proto.state_dict().items()}, seed=11)
    f0 = g['f0']
    b, _, h, w = f0.shape
    x = tok(f0).double()
    q = x @ sd['q_proj.weight'].double().t() + sd['q_proj.bias'].double()
    k_glob = q @ sd['k_proj.weight'].double().t() + sd['k_proj.bias'].double()
    k_loc = x @ sd['k_proj.weight'].double().t() + sd['k_proj.bias'].double()
    for vch in (2, 1):
        val = g[f'val{vch}']
        got = ops.prop_global(q.float().to(DEV), k_glob.float().to(DEV), val.to(DEV), h, w)
        assert err(got, g[f'global{vch}'])[0] < 2e-4
        for r in (1, 2):
            got = ops.prop_local(q.float().to(DEV), k_loc.float().to(DEV), val.to(DEV), h, w, r)
            assert err(got, g[f'local{vch}_r{r}'])[0] < 2e-4


# ------------------------------------------------------------------ local kernels
@pytest.mark.parametrize('tag', ['soft', 'peaky'])
def test_local_kernels_golden(ops, golden, tag):
    g = golden('matching')
    f0, f1 = g[f'{tag}.f0'], g[f'{tag}.f1']
    b, _, h, w = f0.shape
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    for r in (4, 2):
        assert err(ops.local_corr_softmax(t0, t1, h, w, r), g[f'{tag}.local_flow_r{r}'])[0] < 2e-4
        got = ops.local_corr_with_flow(t0, t1, g[f'{tag}.flow_in'].to(DEV), h, w, r)
        want = hp.local_corr_with_flow(f0.double(), f1.double(), g[f'{tag}.flow_in'].double(), r)
        assert err(got, want)[0] < 1e-4 * max(1.0, want.abs().max().item())
        assert err(got, g[f'{tag}.cost_r{r}'])[0] < 2e-4 * max(1.0, want.abs().max().item())
    assert err(ops.local_corr_softmax(t0, t1, h, w, 4, one_d=True), g[f'{tag}.stereo_local_r4'])[0] < 2e-4
    # depth
    k, pose, cand = g[f'{tag}.K'], g[f'{tag}.pose'], g[f'{tag}.cand']
    cam = torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1)
    got = ops.depth_corr_softmax(t0, t1, h, w, cam.contiguous().to(DEV), cand.to(DEV))
    assert err(got, g[f'{tag}.depth'])[0] < 2e-4
    got = ops.depth_corr_softmax(t0, t1, h, w, cam.contiguous().to(DEV), cand.to(DEV), from_argmax=True)
    assert (got.cpu() - g[f'{tag}.depth_argmax']).abs().gt(1e-6).float().mean().item() < 0.01


def _random_local_cases(count, seed=31):
    import random
    rng = random.Random(seed)
    out = [(1, 1, 1, 1), (1, 2, 9, 4), (2, 9, 2, 3)]                 # one pixel; maps smaller than the window
    while len(out) < count:
        out.append((rng.choice([1, 2, 3]), rng.randrange(3, 34), rng.randrange(3, 50), rng.choice([1, 2, 3, 4])))
    return out


@pytest.mark.parametrize('case', _random_local_cases(16))
def test_local_kernels_random_shapes(ops, case):
    """Local correlation softmax (2-D and 1-D), the flow-displaced cost volume (fractional, exactly integer and far
    out-of-image flow) and the plane-sweep depth correlation against the fp64 oracle over pseudo-random map sizes and
    radii -- whichever kernel serves the shape (matrix-core or gather path)."""
    b, h, w, r = case
    f0, f1 = rnd(500 + h, b, C, h, w), rnd(501 + w, b, C, h, w)
    f1 = 0.5 * f0.roll((1, 1), (2, 3)) + 0.5 * f1
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    for one_d in (False, True):
        want = hp.local_corr_softmax(f0.double(), f1.double(), r, one_d)
        assert err(ops.local_corr_softmax(t0, t1, h, w, r, one_d=one_d), want)[0] < 2e-4, (case, one_d)
    flow = rnd(502, b, 2, h, w, scale=2.5)
    flow[:, :, 0, 0] = 3.0                                              # exactly integer displacement
    flow[:, :, -1, -1] = 1000.0                                         # far outside: all zeros
    want = hp.local_corr_with_flow(f0.double(), f1.double(), flow.double(), r)
    got = ops.local_corr_with_flow(t0, t1, flow.to(DEV), h, w, r)
    assert err(got, want)[0] < 1e-4 * max(1.0, want.abs().max().item()), case
    # depth: a sideways camera move, candidates that project inside and outside of the map
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    pose[:, :3, 3] = torch.tensor([0.12, -0.03, 0.02])
    cand = torch.linspace(1 / 10.0, 1 / 0.5, 24)
    want = hp.depth_corr_softmax(f0.double(), f1.double(), k.double(), pose.double(), cand.double())
    cam = torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1)
    got = ops.depth_corr_softmax(t0, t1, h, w, cam.contiguous().to(DEV), cand.to(DEV))
    assert err(got, want)[0] < 2e-4 * max(1.0, want.abs().max().item()), case


@pytest.mark.parametrize('case', ['sideways', 'diagonal', 'forward', 'many_candidates', 'argmax'])
def test_plane_sweep_box_and_gather_paths(ops, case):
    """um_depth_corr_softmax (matching.py:203-282) through all of its paths against the fp64 oracle: the integer-neighbourhood form
    (lane = candidate, dots with the distinct f1 rows of the candidates' bounding box, blended from a wave-private table) for a
    sideways move; a long DIAGONAL epipolar segment whose box exceeds the table (per-pixel gather fallback inside the same kernel);
    a forward move (epipolar lines radiate from the centre: boxes of every shape, candidates leaving the image); more than 64
    candidates (the gather kernel); and the arg-max read-out (first index attaining the maximum)."""
    b, h, w = 2, 30, 40
    f0, f1 = rnd(1500, b, C, h, w), rnd(1501, b, C, h, w)
    f1 = 0.6 * f0.roll((0, 2), (2, 3)) + 0.4 * f1
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    nd, argmax = 64, False
    if case == 'sideways':
        pose[:, :3, 3] = torch.tensor([0.12, -0.01, 0.0])
    elif case == 'diagonal':
        pose[:, :3, 3] = torch.tensor([0.45, 0.40, 0.0])              # ~30 x 27 cells between the first and the last candidate
    elif case == 'forward':
        pose[:, :3, 3] = torch.tensor([0.02, 0.01, 0.30])
        ang = 0.04
        pose[1, :3, :3] = torch.tensor([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1.0]])
    elif case == 'many_candidates':
        pose[:, :3, 3] = torch.tensor([0.12, -0.03, 0.02])
        nd = 80
    else:
        pose[:, :3, 3] = torch.tensor([0.10, 0.02, 0.01])
        argmax = True
    cand = torch.linspace(1 / 10.0, 1 / 0.5, nd)
    want = hp.depth_corr_softmax(f0.double(), f1.double(), k.double(), pose.double(), cand.double(), argmax)
    cam = torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1)
    got = ops.depth_corr_softmax(t0, t1, h, w, cam.contiguous().to(DEV), cand.to(DEV), from_argmax=argmax)
    assert torch.isfinite(got).all()
    if argmax:                                                          # ties / near-ties may pick a neighbouring candidate
        assert (got.cpu().double() - want).abs().gt(1e-6).float().mean().item() < 0.01
    else:
        assert err(got, want)[0] < 2e-4 * max(1.0, want.abs().max().item()), (case, err(got, want))


def test_cost_volume_config4_size_properties(ops):
    """At config-4's scale-1 size (128x192): zero flow -> the centre tap equals the plain per-pixel
    correlation f0.f1/sqrt(C), and an integer flow only shifts which tap that is (bilinear weights 1,0,0,0)."""
    b, h, w = 2, 128, 192
    f0, f1 = rnd(60, b, C, h, w), rnd(61, b, C, h, w)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    plain = ((f0 * f1).sum(1) / math.sqrt(C)).to(DEV)
    cost = ops.local_corr_with_flow(t0, t1, torch.zeros(b, 2, h, w, device=DEV), h, w, 4)
    assert cost.shape == (b, 81, h, w)
    assert (cost[:, 40] - plain).abs().max().item() < 1e-4
    flow = torch.zeros(b, 2, h, w, device=DEV)
    flow[:, 0] = 2.0
    flow[:, 1] = -1.0
    cost2 = ops.local_corr_with_flow(t0, t1, flow, h, w, 4)
    # tap (dy=+1, dx=-2) of the displaced volume looks at p again
    assert (cost2[:, (1 + 4) * 9 + (-2 + 4)] - plain).abs().max().item() < 1e-4


# ------------------------------------------------------------------ end to end through the drop-in module
SIZES = {'gmflow_s1': (64, 96), 'gmstereo_s1': (64, 96), 'gmdepth_s1': (96, 128), 'gmdepth_s1_rr1': (96, 128),
         'gmflow_s2_rr6': (128, 192), 'gmstereo_s2_rr3': (128, 192)}


def run_product(name, precision='exact', extra=None, batch=1):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    sd = synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02)
    model.load_state_dict(sd)
    model = model.to(DEV).set_precision(precision)
    hh, ww = SIZES[name]
    i0, i1 = synth_images(batch, hh, ww, seed=1000, kind='shift', normalized=(fk['task'] != 'flow'))
    kw = dict(fk)
    if extra:
        kw.update(extra)
    okw = dict(kw)
    if fk['task'] == 'depth':
        k, pose = synth_camera(batch, hh, ww)
        kw.update(intrinsics=k.to(DEV), pose=pose.to(DEV))
        okw.update(intrinsics=k.double(), pose=pose.double())
    pred = model(i0.to(DEV), i1.to(DEV), **kw)['flow_preds'][0]
    okw.update(num_scales=ck['num_scales'], upsample_factor=ck['upsample_factor'], reg_refine=ck['reg_refine'])
    truth = om.unimatch_forward(sd, i0.double(), i1.double(), **okw)
    ref32 = om.unimatch_forward(sd, i0, i1, **{k: (v.float() if torch.is_tensor(v) else v) for k, v in okw.items()})
    return pred.cpu(), truth, ref32


@pytest.mark.parametrize('name', sorted(SIZES))
def test_end_to_end_exact_mode(name, golden):
    """Whole forward on the GPU vs an fp64 evaluation.  The bar: the HIP path (exact mode) may be at most
    3x as far from the fp64 truth as the fp32 CPU oracle is (+1e-4 slack); for the well-conditioned
    single-scale configs that is far below the 1e-3 EPE gate, and the reference's own fp32 output stored in
    the fixture must be within 1e-3 mean as well."""
    pred, truth, ref32 = run_product(name)
    assert pred.shape == truth.shape
    e_new = (pred.double() - truth).abs().mean().item()
    e_ref = (ref32.double() - truth).abs().mean().item()
    assert e_new < 3 * e_ref + 1e-4, (name, e_new, e_ref)
    if 's2' not in name:
        g = golden('e2e')
        assert (pred - g[f'{name}.fp32']).abs().mean().item() < 1e-3


def test_end_to_end_bidirectional_and_batch(golden):
    pred, truth, _ = run_product('gmflow_s1', extra=dict(pred_bidir_flow=True))
    assert pred.shape == (2, 2, 64, 96)
    assert (pred.double() - truth).abs().mean().item() < 1e-3
    assert (pred - golden('e2e')['gmflow_s1_bidir.fp32']).abs().mean().item() < 1e-3
    pred, truth, _ = run_product('gmdepth_s1', extra=dict(pred_bidir_depth=True))
    assert (pred.double() - truth).abs().mean().item() < 1e-4
    pred, truth, _ = run_product('gmflow_s1', batch=3)
    assert (pred.double() - truth).abs().mean().item() < 1e-3


def test_fast_mode_runs_and_is_in_the_ballpark():
    pred, truth, _ = run_product('gmflow_s1', precision='fast')
    assert torch.isfinite(pred).all()
    assert (pred.double() - truth).abs().mean().item() < 2.0     # bf16 operands: px-level, reported not gated


# ------------------------------------------------------------------ fused Transformer-layer tail (um_linear_fwd)
def _planes_to_float(planes, m, n, nplanes):
    halves = planes.view(torch.float16 if nplanes == 2 else torch.bfloat16).view(nplanes, m, n).float()
    return halves.sum(0)


@pytest.mark.parametrize('mk', [(300, 128, 128), (257, 384, 128), (128, 1024, 256)])
def test_linear_planes_and_gelu(ops, mk):
    """A . W^T written as operand planes (ragged M, fused q|k|v width, FFN width with the K-concatenated input
    and the erf-GELU epilogue) against fp64.  Tolerance: the planes carry 22 bits, the product is fp32-accurate."""
    m, n, k = mk
    a = rnd(70, m, k, scale=2.0)
    w = rnd(71, n, k, scale=0.1)
    want = a.double() @ w.double().t()
    if k == 256:
        a0, a1 = a[:, :128].contiguous(), a[:, 128:].contiguous()
        got, _, _ = ops.linear_planes(a0.to(DEV), (w.to(DEV),), a1=a1.to(DEV), gelu=True)
        want = torch.nn.functional.gelu(want)
    else:
        chunks = tuple(x.contiguous().to(DEV) for x in w.split(128, 0))
        got, _, _ = ops.linear_planes(a.to(DEV), chunks)
    got = _planes_to_float(got.cpu(), m, n, 2)
    assert (got.double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_linear_layernorm_residual(ops):
    m = 333
    a = rnd(72, m, 128, scale=2.0)
    w = rnd(73, 128, 128, scale=0.1)
    res = rnd(74, m, 128)
    norm = torch.nn.LayerNorm(128)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(75, 128))
        norm.bias.copy_(0.1 * rnd(76, 128))
    want = torch.nn.functional.layer_norm(a.double() @ w.double().t(), (128,), norm.weight.double(), norm.bias.double(),
                                          norm.eps)
    norm = norm.to(DEV)
    got = ops.linear_ln(a.to(DEV), (w.to(DEV),), norm)
    assert err(got, want)[0] < 2e-5
    got = ops.linear_ln(a.to(DEV), (w.to(DEV),), norm, residual=res.to(DEV))
    assert err(got, want + res.double())[0] < 2e-5
    # planes input (the FFN's second GEMM): K = 1024
    hid = rnd(77, m, 1024)
    w2 = rnd(78, 128, 1024, scale=0.05)
    ident = torch.eye(1024)
    hp_, _, _ = ops.linear_planes(hid.to(DEV), tuple(x.contiguous().to(DEV) for x in ident.split(128, 0)))   # hid as planes
    got = ops.linear_ln(hp_, (w2.to(DEV),), norm, residual=res.to(DEV), a_planes_k=1024)
    want = torch.nn.functional.layer_norm(hid.double() @ w2.double().t(), (128,), norm.weight.double().cpu(),
                                          norm.bias.double().cpu(), norm.eps) + res.double()
    assert err(got, want)[0] < 5e-5


@pytest.mark.parametrize('m,hidden', [(128, 1024), (333, 1024), (1000, 64), (4096 + 17, 512)])
def test_fused_ffn_kernel(ops, m, hidden):
    """um_ffn_fwd: x + LayerNorm(W2 . gelu(W1 . [x | y])) in one kernel against fp64 (ragged M, several hidden
    widths), and against the two-launch form it replaces.  Tolerance: fp32-accurate (the planes carry 22 bits)."""
    x, y = rnd(80, m, 128, scale=1.5), rnd(81, m, 128, scale=1.5)
    w1 = rnd(82, hidden, 256, scale=0.08)
    w2 = rnd(83, 128, hidden, scale=0.06)
    norm = torch.nn.LayerNorm(128)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(84, 128))
        norm.bias.copy_(0.1 * rnd(85, 128))
    hid = torch.nn.functional.gelu(torch.cat([x, y], 1).double() @ w1.double().t())
    want = x.double() + torch.nn.functional.layer_norm(hid @ w2.double().t(), (128,), norm.weight.double(),
                                                       norm.bias.double(), norm.eps)
    norm = norm.to(DEV)
    xd, yd, w1d, w2d = x.to(DEV), y.to(DEV), w1.to(DEV), w2.to(DEV)
    got = ops.ffn_ln(xd, yd, w1d, w2d, norm)
    assert torch.isfinite(got).all()
    assert err(got, want)[0] < 3e-5
    if hidden % 128 == 0:                         # the two-launch form needs full 128-wide output tiles
        hp_, _, nh = ops.linear_planes(xd, (w1d,), a1=yd, gelu=True)
        two = ops.linear_ln(hp_, (w2d,), norm, residual=xd, a_planes_k=nh)
        assert err(got, two)[0] < 2e-5
    # the bf16 throughput mode runs the same main loop with one operand plane and one product (other gap counts in the software
    # pipeline: round 4's re-ordered loop first lost the accumulator hand-over there): bf16-level agreement with fp64
    fast = HipOps('fast').ffn_ln(xd, yd, w1d, w2d, norm)
    assert torch.isfinite(fast).all() and err(fast, want)[1] < 2e-2 and err(fast, want)[0] < 0.5, err(fast, want)


def test_fused_ffn_rejects_bad_arguments(ops):
    x = rnd(86, 64, 128).to(DEV)
    norm = torch.nn.LayerNorm(128).to(DEV)
    with pytest.raises(ValueError):
        ops.ffn_ln(x, x, rnd(87, 1024, 128).to(DEV), rnd(88, 128, 1024).to(DEV), norm)     # W1 must be [hidden, 256]
    with pytest.raises(Exception):
        ops.ffn_ln(x, x, rnd(87, 48, 256).to(DEV), rnd(88, 128, 48).to(DEV), norm)         # hidden % 32 != 0


# ------------------------------------------------------------------ NHWC convolutions + encoder glue
def _nhwc_planes(ops, x_nchw):
    """NCHW fp32 (CPU) -> the library's NHWC operand planes via um_nchw_to_nhwc."""
    planes, f32 = ops.nchw_to_nhwc(x_nchw.to(DEV).contiguous(), want_planes=True, want_f32=True)
    return planes, f32


@pytest.mark.parametrize('case', [
    # b, cin, cout, h, w, kh, kw, stride, ph, pw, bias, relu
    (2, 64, 64, 20, 28, 3, 3, 1, 1, 1, False, False),        # encoder layer1
    (1, 64, 96, 21, 30, 3, 3, 2, 1, 1, False, False),        # stride 2, odd size
    (2, 96, 96, 9, 13, 3, 3, 1, 1, 1, False, True),          # NT = 3 tile, fused ReLU
    (2, 96, 96, 19, 23, 3, 3, 1, 1, 1, True, True),          # NT = 3, row-window kernel, ragged last tile
    (3, 64, 64, 16, 24, 3, 3, 1, 1, 1, False, False),        # row-window kernel, tiles straddle rows and images
    (1, 64, 64, 40, 7, 3, 3, 1, 1, 1, False, False),         # row-window kernel, image rows much shorter than a tile
    (1, 64, 96, 16, 24, 1, 1, 2, 0, 0, True, False),         # 1x1 projection shortcut with bias
    (1, 128, 128, 8, 12, 3, 3, 1, 1, 1, False, False),       # NT = 4
    (1, 128, 256, 7, 9, 3, 3, 1, 1, 1, True, True),          # two output tiles (flow head / mask head shape)
    (1, 256, 128, 6, 10, 1, 5, 1, 0, 2, True, False),        # SepConvGRU horizontal
    (1, 256, 128, 10, 6, 5, 1, 1, 2, 0, True, False),        # SepConvGRU vertical
    (1, 32, 68, 5, 7, 7, 7, 1, 3, 3, True, False),           # 7x7, ragged cout
    (1, 128, 128, 17, 19, 3, 3, 1, 1, 1, False, False),      # NT = 4 row window (16-channel stages), ragged second tile
    (2, 128, 256, 16, 20, 3, 3, 1, 1, 1, True, True),        # NT = 4 row window, two output tiles, two images
    (2, 256, 128, 18, 15, 1, 5, 1, 0, 2, True, False),       # GRU 1x5 gate shape: five-tap row window
    (1, 256, 256, 9, 40, 1, 5, 1, 0, 2, True, False),        # GRU z|r shape, rows longer than the taps reach
    (1, 64, 64, 33, 65, 3, 3, 1, 1, 1, True, True),          # NT = 2 row window, 9 tiles with a ragged tail
    (2, 64, 64, 16, 64, 3, 3, 1, 1, 1, False, False),        # 2-D patch kernel: 2 x 2 tiles per image, two images
    (1, 64, 36, 8, 32, 3, 3, 1, 1, 1, True, True),           # patch kernel, a single tile (all four borders), ragged cout
    (1, 96, 64, 24, 96, 3, 3, 1, 1, 1, True, False),         # patch kernel, six channel chunks, 3 x 3 tiles (an interior one)
    (1, 128, 128, 24, 32, 3, 3, 1, 1, 1, False, True),       # patch kernel NT = 4
    (2, 96, 96, 16, 32, 3, 3, 1, 1, 1, True, True),          # patch kernel NT = 3 (epilogue in two passes)
    (2, 64, 64, 22, 60, 3, 3, 1, 1, 1, False, False),        # patch kernel, ragged right and bottom tiles
    (1, 128, 128, 15, 90, 3, 3, 1, 1, 1, True, True),        # patch kernel NT = 4, ragged
    (1, 96, 96, 30, 31, 3, 3, 1, 1, 1, True, False),         # patch kernel NT = 3, one ragged column of tiles
    (2, 128, 256, 8, 64, 3, 3, 1, 1, 1, True, True),         # patch kernel NT = 4, two output tiles
])
def test_conv2d_nhwc_matches_fp64(ops, case):
    """um_conv2d_fwd (implicit GEMM on split-fp16 planes) against torch conv2d in fp64: every kernel geometry the
    encoder and the refinement block use; zero padding comes from the planes' zero row."""
    b, cin, cout, h, w, kh, kw, stride, ph, pw, bias, relu = case
    x = rnd(90, b, cin, h, w, scale=1.5)
    wt = rnd(91, cout, cin, kh, kw, scale=(2.0 / (cin * kh * kw)) ** 0.5)
    bs = rnd(92, cout) if bias else None
    want = torch.nn.functional.conv2d(x.double(), wt.double(), bs.double() if bias else None, stride=stride, padding=(ph, pw))
    if relu:
        want = want.relu()
    planes, _ = _nhwc_planes(ops, x)
    got, ho, wo = ops.conv2d_nhwc((planes, b, h, w, cin), wt.to(DEV), bs.to(DEV) if bias else None, stride, (ph, pw), relu)
    assert (ho, wo) == tuple(want.shape[-2:])
    got = got.view(b, ho, wo, cout).permute(0, 3, 1, 2)
    assert err(got, want)[0] < 3e-6 * max(1.0, want.abs().max().item())


def test_cost_volume_planes_equal_the_volume(ops):
    """um_local_corr_with_flow_planes writes the same numbers as um_local_corr_with_flow, channels-last, as fp16 hi + lo
    planes with zero padding channels and an untouched zero row (smooth flow -> four-pixel blocked path, noisy flow ->
    pixel-by-pixel path)."""
    b, h, w = 2, 14, 22
    f0, f1 = rnd(120, b, h * w, 128).to(DEV), rnd(121, b, h * w, 128).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    smooth = torch.stack([2.3 * torch.sin(yy / 5.0) + 0.05 * xx, 1.7 * torch.cos(xx / 7.0)], 0)[None].repeat(b, 1, 1, 1)
    for flow in (smooth.float().contiguous(), rnd(122, b, 2, h, w, scale=3.0)):
        vol = ops.local_corr_with_flow(f0, f1, flow.to(DEV), h, w, 4)                       # [b, 81, h, w]
        rows = b * h * w
        buf = ops.planes_buffer(rows, 96)
        ops.local_corr_with_flow_planes(f0, f1, flow.to(DEV), h, w, 4, buf, 96)
        pl = buf.view(torch.float16).view(2, rows + 1, 96).float()
        got = pl.sum(0)[:rows, :81].view(b, h, w, 81).permute(0, 3, 1, 2)
        assert (got - vol).abs().max().item() < 2e-6 * max(1.0, vol.abs().max().item())
        assert torch.equal(pl[:, :rows, 81:], torch.zeros(2, rows, 15, device=DEV))
        assert torch.equal(pl[:, rows], torch.zeros(2, 96, device=DEV))


def test_cost_volume_planes_validate_flow_and_destination(ops):
    """local_corr_with_flow_planes takes its batch from f0, so it checks ``flow`` against it as local_corr_with_flow does (the
    refinement block at batch 2B on B feature samples was the silent case), and ``dest`` against the rows the kernel writes.  Only
    arguments that would be harmless without the check are tried: a flow with MORE samples than f0, a float64 flow, one channel, a
    destination of another dtype -- every one a ValueError before any launch."""
    b, h, w = 2, 6, 8
    f0, f1 = rnd(123, b, h * w, 128).to(DEV), rnd(124, b, h * w, 128).to(DEV)
    flow = rnd(125, b, 2, h, w).to(DEV)
    buf = ops.planes_buffer(b * h * w, 96)
    ops.local_corr_with_flow_planes(f0, f1, flow, h, w, 4, buf, 96)            # the valid call goes through
    for bad in (torch.cat([flow, flow], 0), flow.double(), flow[:, :1].contiguous()):
        with pytest.raises(ValueError, match='flow'):
            ops.local_corr_with_flow_planes(f0, f1, bad, h, w, 4, buf, 96)
    with pytest.raises(ValueError, match='dest'):
        ops.local_corr_with_flow_planes(f0, f1, flow, h, w, 4, ops.planes_buffer(b * h * w, 96).view(torch.float16), 96)


@pytest.mark.parametrize('hw', [(9, 11), (16, 32)])                # generic kernel; 2-D patch kernel (whole 8 x 32 tiles)
def test_conv_ex_offsets_and_gates(ops, hw):
    """um_conv2d_ex reading a column slice and writing planes at a column offset (the block's concat-free chaining), and
    the three um_nhwc_gate modes against plain tensor arithmetic."""
    b, (h, w), cin, cout = 2, hw, 64, 128
    rows = b * h * w
    x = rnd(123, rows, 96)                                                       # the conv reads columns 32..96 of this
    wt = rnd(124, cout, cin, 3, 3, scale=0.05)
    bs = rnd(125, cout)
    src = ops.planes_buffer(rows, 96)
    ops.nhwc_gate(0, x.to(DEV), src, 96, 0, rows, 96)
    dst = ops.planes_buffer(rows, 256)
    f32 = torch.zeros((rows, 160), dtype=torch.float32, device=DEV)
    wb = (ops.conv_weight_planes_from(wt.to(DEV)), bs.to(DEV))
    ops.conv_ex((src, 96, 32, cin), (b, h, w), wb, (3, 3), 1, (1, 1), 3, out=(f32, 160, 32), outp=(dst, 256, 128))
    xin = x[:, 32:].view(b, h, w, cin).permute(0, 3, 1, 2).double()
    want = torch.tanh(torch.nn.functional.conv2d(xin, wt.double(), bs.double(), padding=1)).permute(0, 2, 3, 1).reshape(rows, cout)
    assert err(f32[:, 32:], want)[0] < 3e-6
    assert torch.equal(f32[:, :32], torch.zeros(rows, 32, device=DEV))                       # untouched columns
    pl = dst.view(torch.float16).view(2, rows + 1, 256).float().sum(0)
    assert err(pl[:rows, 128:], want)[0] < 3e-6 and torch.equal(pl[:rows, :128], torch.zeros(rows, 128, device=DEV))
    # gates: r * h and the state update
    zr = torch.sigmoid(rnd(126, rows, 256)).to(DEV)
    hb = rnd(127, rows, 128).to(DEV)
    q = torch.tanh(rnd(128, rows, 128)).to(DEV)
    g = ops.planes_buffer(rows, 512)
    ops.nhwc_gate(1, None, g, 512, 384, rows, 128, zr=zr, hbuf=hb)
    got = g.view(torch.float16).view(2, rows + 1, 512).float().sum(0)[:rows, 384:]
    assert (got - zr[:, 128:] * hb).abs().max().item() < 1e-6
    want_h = (1 - zr[:, :128]) * hb + zr[:, :128] * q
    ops.nhwc_gate(2, q, g, 512, 0, rows, 128, zr=zr, hbuf=hb)
    assert (hb - want_h).abs().max().item() < 1e-6
    got = g.view(torch.float16).view(2, rows + 1, 512).float().sum(0)[:rows, :128]
    assert (got - hb).abs().max().item() < 1e-6
    # ragged column scatter (flow: 2 channels at an even offset)
    fl = rnd(129, rows, 2).to(DEV)
    ops.nhwc_gate(0, fl, g, 512, 382, rows, 2)
    got = g.view(torch.float16).view(2, rows + 1, 512).float().sum(0)[:rows, 382:384]
    assert (got - fl).abs().max().item() < 1e-6


def test_flow_warp(ops):
    """um_flow_warp against the oracle's grid_sample warp in fp64: sub-pixel offsets, samples leaving the image on every
    side (zeros padding), exact integer offsets."""
    b, h, w, c = 2, 13, 17, 128
    feat = rnd(110, b, c, h, w)
    flow = rnd(111, b, 2, h, w, scale=4.0)
    flow[0, :, :3] = torch.tensor([2.0, -1.0]).view(2, 1, 1)          # integer offsets
    flow[1, :, -2:] = 40.0                                             # far outside
    want = om.warp(feat.double(), flow.double())
    tok = feat.flatten(2).transpose(1, 2).contiguous()
    got = ops.flow_warp(tok.to(DEV), flow.to(DEV), h, w).transpose(1, 2).reshape(b, c, h, w)
    assert err(got, want)[0] < 2e-5


@pytest.mark.parametrize('fd,hw', [(2, (16, 24)), (1, (12, 20))])
def test_nhwc_update_block_matches_module(ops, fd, hw):
    """The channels-last refinement block (refine_nhwc.NhwcUpdateBlock: K4 -> planes, concat-free convolution chain, fused
    gates) against the stock BasicUpdateBlock module evaluated in fp64 on the same weights and inputs."""
    from unimatch_amd.refine import BasicUpdateBlock
    from unimatch_amd.refine_nhwc import NhwcUpdateBlock
    torch.manual_seed(5)
    b, (h, w) = 2, hw
    block = BasicUpdateBlock(corr_channels=81, downsample_factor=4, flow_dim=fd)
    proj = torch.nn.Conv2d(128, 256, 1)
    f0 = rnd(101, b, h * w, 128)
    ori0, ori1 = rnd(102, b, h * w, 128), rnd(103, b, h * w, 128)
    flow = rnd(104, b, fd, h, w, scale=2.0)
    disp = torch.cat([-flow, torch.zeros_like(flow)], 1) if fd == 1 else flow
    # fp64 reference with the oracle's cost volume
    blk64, proj64 = BasicUpdateBlock(81, downsample_factor=4, flow_dim=fd).double(), torch.nn.Conv2d(128, 256, 1).double()
    blk64.load_state_dict({k: v.double() for k, v in block.state_dict().items()})
    proj64.load_state_dict({k: v.double() for k, v in proj.state_dict().items()})
    with torch.no_grad():
        fmap = f0.double().transpose(1, 2).reshape(b, 128, h, w)
        p64 = proj64(fmap)
        net0, inp = torch.tanh(p64[:, :128]), torch.relu(p64[:, 128:])
        corr = hp.local_corr_with_flow(ori0.double().transpose(1, 2).reshape(b, 128, h, w),
                                       ori1.double().transpose(1, 2).reshape(b, 128, h, w), disp.double(), 4)
        _, mask64, delta64 = blk64(net0, inp, corr, flow.double())
    block, proj = block.to(DEV), proj.to(DEV)
    upd = NhwcUpdateBlock(ops, block, proj)
    upd.begin(f0.to(DEV), b, h, w)
    mask, delta = upd.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert err(delta, delta64)[0] < 2e-5 * max(1.0, delta64.abs().max().item())
    got_mask = mask.view(b, h, w, -1).permute(0, 3, 1, 2)
    assert err(got_mask, mask64)[0] < 2e-5 * max(1.0, mask64.abs().max().item())
    # a second iteration must not depend on state left by the first (the hidden state restarts from net0)
    mask2, delta2 = upd.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert torch.equal(delta2, delta) and torch.equal(mask2, mask)
    # round 4: with more than one iteration announced, the iteration-invariant share of the four gate convolutions (context
    # features, initial hidden state: unimatch.py:315-331) is computed once in begin() and enters the per-iteration convolutions as
    # their epilogue's addend (um_conv2d_gru_add_fwd): same result up to fp32 summation order, again independent of earlier iterations
    assert not upd.hoist
    hst = NhwcUpdateBlock(ops, block, proj)
    hst.begin(f0.to(DEV), b, h, w, iterations=3)
    assert hst.hoist
    mask_h, delta_h = hst.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert err(delta_h, delta64)[0] < 2e-5 * max(1.0, delta64.abs().max().item())
    assert err(mask_h.view(b, h, w, -1).permute(0, 3, 1, 2), mask64)[0] < 2e-5 * max(1.0, mask64.abs().max().item())
    assert err(delta_h, delta)[0] < 1e-5 * max(1.0, delta64.abs().max().item())
    flow2 = flow + 0.25
    disp2 = torch.cat([-flow2, torch.zeros_like(flow2)], 1) if fd == 1 else flow2
    hst.iterate(ori0.to(DEV), ori1.to(DEV), disp2.to(DEV).contiguous(), flow2.to(DEV), False)      # another input in between
    mask_h2, delta_h2 = hst.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert torch.equal(delta_h2, delta_h) and torch.equal(mask_h2, mask_h)
    # the six activation plane buffers are allocated and zeroed once per geometry and owner (ops.cached_planes_buffer) and handed
    # out again by every begin(): nothing may be read that this forward has not written -- poison every row but the zero padding
    # row with fp16 NaNs (0xffff) and run the forward again
    planes = {k: v for k, v in ops.workspace_entries() if isinstance(k.kind, tuple) and k.geometry[0] == b * h * w}
    assert {k.kind[1] for k in planes} == {'G', 'C1', 'CF', 'FH', 'F1', 'CORR'}
    def poison():
        for key, buf in planes.items():
            rows, ld = key.geometry
            buf.view(torch.int16).view(2, rows + 1, ld)[:, :rows].fill_(-1)

    poison()
    hst.begin(f0.to(DEV), b, h, w, iterations=3)
    mask_h3, delta_h3 = hst.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert torch.equal(delta_h3, delta_h) and torch.equal(mask_h3, mask_h)
    poison()
    upd.begin(f0.to(DEV), b, h, w)
    mask3, delta3 = upd.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert torch.equal(delta3, delta) and torch.equal(mask3, mask)
    # the hoisted gate share must cover every pixel row: a short addend is an error, not an out-of-bounds read
    with pytest.raises(ValueError, match='addend must be'):
        ops.conv_gru(1, (hst.G, 512, 256, 128), (b, h, w), hst.wts['zr1v'], (1, 5), (0, 2), hst.H, (hst.G, 512, 384), z_out=hst.ZR,
                     addend=hst.P['zr1'][:-1].contiguous())
    # explicit release of the cached activation planes (~590 MB per stream at config 4): gone from the cache, rebuilt on demand
    ops.release_cached_planes()
    assert not [k for k, _ in ops.workspace_entries() if isinstance(k.kind, tuple)]
    upd.begin(f0.to(DEV), b, h, w)
    mask4, delta4 = upd.iterate(ori0.to(DEV), ori1.to(DEV), disp.to(DEV).contiguous(), flow.to(DEV), True)
    assert torch.equal(delta4, delta) and torch.equal(mask4, mask)


@pytest.mark.parametrize('bhw,normalize', [((2, 64, 96), True), ((1, 37, 51), False), ((3, 16, 32), True)])
def test_stem_conv_matches_fp64(ops, bhw, normalize):
    """um_stem_conv_fwd: the 7x7 / stride 2 / pad 3 stem through the packed NHWC-4 image planes against torch conv2d in
    fp64 (even and odd sizes), with and without the reference's input normalisation folded into the packing."""
    b, h, w = bhw
    img = rnd(99, b, 3, h, w).abs() * 120.0 if normalize else rnd(99, b, 3, h, w, scale=2.0)
    wt = rnd(100, 64, 3, 7, 7, scale=0.12)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    x = img.double()
    if normalize:
        x = (x / 255.0 - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    want = torch.nn.functional.conv2d(x, wt.double(), None, stride=2, padding=3)
    got, ho, wo = ops.stem_conv(img.to(DEV).contiguous(), wt.to(DEV), (mean, std) if normalize else None)
    assert (ho, wo) == tuple(want.shape[-2:])
    got = got.view(b, ho, wo, 64).permute(0, 3, 1, 2)
    assert err(got, want)[0] < 4e-6 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('cout,hw,stride', [(64, (16, 24), 1), (96, (32, 12), 1), (256, (8, 16), 1),
                                            (64, (15, 21), 1),        # 315 pixels: ragged third tile (row-window kernel)
                                            (128, (19, 23), 1),       # NT = 4: generic kernel, 437 pixels
                                            (96, (7, 9), 1),          # 63 pixels: a single partial tile per image
                                            (96, (21, 30), 2),        # stride 2 -> 11 x 15 = 165 pixels
                                            (64, (16, 64), 1),        # 2-D patch kernel: parts in tile order
                                            (128, (24, 32), 1),       # patch kernel NT = 4
                                            (96, (16, 64), 1),        # patch kernel NT = 3
                                            (64, (22, 60), 1),        # patch kernel, ragged tiles: parts with 0 .. 128 pixels
                                            (96, (30, 31), 1),
                                            (128, (15, 90), 1),
                                            (64, (47, 63), 2)])       # KITTI-like odd map
def test_conv_epilogue_statistics_feed_the_norm(ops, cout, hw, stride):
    """um_conv2d_fwd(stats_out) -> um_nhwc_instance_norm(conv_stats): the per-tile statistics written by the convolution's
    epilogue must give the same normalisation as the fp64 reference (and as the norm's own statistics pass), for any
    number of pixels per image (tiles are per image, the last one ragged)."""
    b, cin, (h, w) = 3, 64, hw
    x = rnd(96, b, cin, h, w, scale=1.5)
    wt = rnd(97, cout, cin, 3, 3, scale=0.06)
    bs = 3.0 * rnd(98, cout)                                   # a large mean per channel
    planes, _ = _nhwc_planes(ops, x)
    y, ho, wo = ops.conv2d_nhwc((planes, b, h, w, cin), wt.to(DEV), bs.to(DEV), stride, (1, 1), stats=True)
    assert ops.last_conv_stats is not None
    _, got = ops.nhwc_norm(y, b, ho * wo, relu=False, want_planes=False, want_f32=True, conv_stats=ops.last_conv_stats)
    _, own = ops.nhwc_norm(y, b, ho * wo, relu=False, want_planes=False, want_f32=True)
    want = torch.nn.functional.instance_norm(
        torch.nn.functional.conv2d(x.double(), wt.double(), bs.double(), stride=stride, padding=1))
    assert err(got.view(b, ho, wo, cout).permute(0, 3, 1, 2), want)[0] < 3e-5
    assert err(got, own)[0] < 1e-5


def _random_conv_cases(n, seed=2024):
    """Deterministic pseudo-random convolution geometries: every kernel family (generic / row-window, all tile widths),
    odd sizes, ragged tiles, non-square kernels and paddings."""
    import random
    rng = random.Random(seed)
    cases = []
    while len(cases) < n:
        kh, kw = rng.choice([(1, 1), (3, 3), (3, 3), (1, 5), (5, 1), (3, 1), (1, 3), (5, 5), (7, 7)])
        stride = rng.choice([1, 1, 1, 2])
        ph, pw = rng.choice([(kh // 2, kw // 2), (kh // 2, kw // 2), (0, 0), (kh // 2, 0), (1, 2)])
        b, h, w = rng.choice([1, 2, 3]), rng.randint(5, 40), rng.randint(5, 40)
        cin = rng.choice([32, 64, 96, 128, 160])
        cout = rng.choice([4, 8, 36, 64, 96, 100, 128, 192, 256])
        if (h + 2 * ph - kh) // stride + 1 < 1 or (w + 2 * pw - kw) // stride + 1 < 1:
            continue
        cases.append((b, cin, cout, h, w, kh, kw, stride, ph, pw, rng.random() < 0.5, rng.choice([0, 1, 2, 3])))
    return cases


@pytest.mark.parametrize('case', _random_conv_cases(28))
def test_conv2d_ex_random_geometries(ops, case):
    """um_conv2d_ex over pseudo-random geometries (kernel shapes, strides, paddings, channel counts, activations) against
    torch conv2d in fp64."""
    b, cin, cout, h, w, kh, kw, stride, ph, pw, bias, act = case
    x = rnd(130, b, cin, h, w, scale=1.2)
    wt = rnd(131, cout, cin, kh, kw, scale=(2.0 / (cin * kh * kw)) ** 0.5)
    bs = rnd(132, cout) if bias else None
    pre = torch.nn.functional.conv2d(x.double(), wt.double(), bs.double() if bias else None, stride=stride, padding=(ph, pw))
    want = (pre, pre.relu(), torch.sigmoid(pre), torch.tanh(pre))[act]
    ho, wo = want.shape[-2:]
    rows_in, rows_out = b * h * w, b * ho * wo
    src = ops.planes_buffer(rows_in, cin)
    ops.nhwc_gate(0, x.permute(0, 2, 3, 1).reshape(rows_in, cin).contiguous().to(DEV), src, cin, 0, rows_in, cin)
    out = torch.empty((rows_out, cout), dtype=torch.float32, device=DEV)
    wb = (ops.conv_weight_planes_from(wt.to(DEV)), bs.to(DEV) if bias else None)
    ops.conv_ex((src, cin, 0, cin), (b, h, w), wb, (kh, kw), stride, (ph, pw), act, out=(out, cout, 0))
    got = out.view(b, ho, wo, cout).permute(0, 3, 1, 2)
    # fp32 accumulation over K = kh*kw*cin terms of 22-bit operand products; the activations have slope <= 1
    assert err(got, want)[0] < 3e-6 * max(1.0, pre.abs().max().item()), case


@pytest.mark.parametrize('shape', [(2, 64, 37, 29), (1, 96, 64, 48), (3, 128, 5, 7),
                                   (1, 8, 520, 512)])      # > 1024 statistics parts per image: the two-pass merge
def test_nhwc_instance_norm(ops, shape):
    """NHWC InstanceNorm (+ ReLU, + shortcut + ReLU) against fp64, both output formats; a large mean exercises the
    shifted statistics.  Planes are checked by summing hi + lo."""
    b, c, h, w = shape
    x = rnd(93, b, c, h, w, scale=2.0) + 30.0 * rnd(94, 1, c, 1, 1)
    sc = rnd(95, b, c, h, w)
    _, xf = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=False, want_f32=True)
    assert torch.equal(xf.view(b, h, w, c).permute(0, 3, 1, 2).cpu(), x)
    _, scf = ops.nchw_to_nhwc(sc.to(DEV).contiguous(), want_planes=False, want_f32=True)
    n64 = torch.nn.functional.instance_norm(x.double())
    for relu, shortcut in ((True, None), (False, None), (True, scf)):
        want = n64.relu() if relu else n64
        if shortcut is not None:
            want = (want + sc.double()).relu()
        planes, f32 = ops.nhwc_norm(xf, b, h * w, relu=relu, shortcut=shortcut, want_planes=True, want_f32=True)
        got = f32.view(b, h, w, c).permute(0, 3, 1, 2)
        assert err(got, want)[0] < 2e-5
        rows = b * h * w
        pl = planes.view(torch.float16).view(2, rows + 1, c).float()
        assert torch.equal(pl[:, rows], torch.zeros(2, c, device=DEV))              # the padding row
        assert (pl[:, :rows].sum(0) - f32).abs().max().item() < 2e-6 * max(1.0, f32.abs().max().item())
    # the shortcut handed over as operand planes (what the encoder does for identity shortcuts): hi + lo is added
    scp, _ = ops.nhwc_norm(scf, b, h * w, normalize=False, relu=False, want_planes=True)
    _, f32 = ops.nhwc_norm(xf, b, h * w, relu=True, shortcut_planes=scp, want_planes=False, want_f32=True)
    want = (n64.relu() + sc.double()).relu()
    assert err(f32.view(b, h, w, c).permute(0, 3, 1, 2), want)[0] < 2e-5


@pytest.mark.parametrize('shifted,residual', [(False, True), (True, False)])
def test_attention_merge_and_kv_rotate(ops, shifted, residual):
    """um_window_attn_merge_fwd with kv_rotate against its composition from separately tested pieces in fp64: attention of
    stream s against the keys / values of stream (s + r) mod S, then merge Linear + LayerNorm (+ residual)."""
    s_, h, w, c = 4, 16, 24, 128
    l = h * w
    x = rnd(140, s_ * l, c, scale=1.5)
    xt = rnd(141, s_ * l, c, scale=1.5)
    wq, wk, wv, wm = (rnd(142 + i, c, c, scale=0.09) for i in range(4))
    norm = torch.nn.LayerNorm(c)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(146, c))
        norm.bias.copy_(0.1 * rnd(147, c))
    geom = (8, 12, 4, 6) if shifted else (8, 12, 0, 0)
    rot = 2
    # fp64 reference: explicit rotation of the key / value streams, oracle attention, merge, LayerNorm
    want = merged_layer_reference(x, xt, wq, wk, wv, wm, norm, s_, h, w, geom, rot, residual)
    norm = norm.to(DEV)
    xd, xtd = x.to(DEV), xt.to(DEV)
    qp, _, _ = ops.linear_planes(xd, (wq.to(DEV),))
    kv, _, n2 = ops.linear_planes(xtd, (wk.to(DEV), wv.to(DEV)))
    m = s_ * l
    got = ops.window_attention_merge((qp, m, c, 0), (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), norm,
                                     xd if residual else None)
    assert err(got.reshape(m, c), want)[0] < 5e-5
    # the same layer with the query projection in the kernel's prologue (um_window_attn_qproj_merge_fwd)
    got2 = ops.window_attention_qproj_merge(xd, wq.to(DEV), (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), norm,
                                            xd if residual else None)
    assert err(got2.reshape(m, c), want)[0] < 5e-5
    fast = HipOps('fast')
    kvf, _, _ = fast.linear_planes(xtd, (wk.to(DEV), wv.to(DEV)))
    qpf, _, _ = fast.linear_planes(xd, (wq.to(DEV),))
    ref_f = fast.window_attention_merge((qpf, m, c, 0), (kvf, m, n2, 0), (kvf, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), norm,
                                        xd if residual else None)
    got_f = fast.window_attention_qproj_merge(xd, wq.to(DEV), (kvf, m, n2, 0), (kvf, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV),
                                              norm, xd if residual else None)
    # bf16 operands: q rounds the same way up to its accumulation order, so the two agree with fp64 equally well (the mean error
    # is the stable statistic: the maximum over 2e5 LayerNorm outputs is a tail event of either evaluation)
    e_ref, e_got = err(ref_f.reshape(m, c), want), err(got_f.reshape(m, c), want)
    assert e_got[1] < 1.25 * e_ref[1] + 1e-4 and e_got[0] < 2.5 * e_ref[0] + 1e-3, (e_ref, e_got)


@pytest.mark.parametrize('geo', [
    (2, 16, 24, 8, 12, 4, 6, 1),        # shifted 2-D windows
    (2, 10, 30, 1, 30, 0, 0, 0),        # 1-D row windows of 30 tokens (ragged: less than one key tile, less than a query tile)
    (2, 12, 20, 12, 20, 0, 0, 1),       # one full window of 240 tokens (ragged last query tile and key tile)
    (4, 6, 10, 3, 5, 1, 2, 2),          # 15-token shifted windows
    (2, 9, 40, 1, 10, 0, 5, 1),         # shifted 1-D windows (swin-1-D)
    (2, 64, 96, 32, 48, 16, 24, 1),     # config-2 size, shifted: token table in LDS, 48 key tiles
    (1, 80, 120, 80, 120, 0, 0, 0),     # 9600-token full window: token table does not fit, arithmetic addressing
    # small launches: the key-split variant (2 or 4 workgroups per query tile, partial softmaxes merged through memory)
    (1, 32, 48, 32, 48, 0, 0, 0),       # 12 query tiles x 48 key tiles: 4 parts
    (2, 40, 56, 20, 28, 10, 14, 1),     # config-1 geometry (560-token shifted windows, ragged last key tile): 4 parts of 4.5 tiles
    (2, 32, 48, 16, 24, 8, 12, 1),      # 384-token shifted windows, 12 key tiles: 2 parts
    (1, 64, 96, 32, 48, 16, 24, 0),     # batch-1 config-2 geometry: 48 query tiles, 2 parts
    # big launches (more than one round of resident workgroups): the instantiation bench.py times
    (16, 64, 96, 32, 48, 16, 24, 8),    # config 2 at batch 8, shifted, cross-attention rotation
    (12, 40, 56, 20, 28, 0, 0, 0),      # 560-token windows (5 query tiles of 128: ragged last tile), 240 tiles ... small launch
    (32, 60, 80, 30, 40, 15, 20, 16),   # config 5 at batch 16: 1200-token windows (ragged key tile), 1280 query tiles
])
def test_query_projection_prologue_matches_q_planes(ops, geo):
    """um_window_attn_qproj_merge_fwd against um_window_attn_merge_fwd fed with q planes from um_linear_fwd, over window
    geometries (ragged tiles, shifts, 1-D windows, both addressing modes): same arithmetic up to the accumulation order of
    q, so the two agree to fp32 rounding of the logits."""
    s_, h, w, wh, ww, sh, sw, rot = geo
    l, c = h * w, 128
    m = s_ * l
    x = rnd(900 + h, m, c, scale=1.5).to(DEV)
    xt = rnd(901 + w, m, c, scale=1.5).to(DEV)
    wq, wk, wv, wm = (rnd(902 + i, c, c, scale=0.09).to(DEV) for i in range(4))
    norm = torch.nn.LayerNorm(c).to(DEV)
    qp, _, _ = ops.linear_planes(x, (wq,))
    kv, _, n2 = ops.linear_planes(xt, (wk, wv))
    ref = ops.window_attention_merge((qp, m, c, 0), (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, wh, ww, sh, sw, rot, wm, norm, x)
    got = ops.window_attention_qproj_merge(x, wq, (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, wh, ww, sh, sw, rot, wm, norm, x)
    assert torch.isfinite(got).all()
    assert err(got, ref)[0] < 2e-5, geo


def test_key_split_launches_skip_masked_tiles_too(ops):
    """Round 6: the key-split small launches (batch 1: the reference's own evaluation protocol) share the walk by rank -- part p of a
    query tile takes the p-th share of the tiles to compute and of the tiles to probe.  Batch-1 config-2 geometry (one stream of 64x96,
    2x2 windows of 1536 tokens, shift 16/24: 48 query tiles x 4 parts): census closed form, result equal to the q-planes kernel's; and
    a masked key that must win the softmax (logit far above its row) is still found by the part whose share it falls into."""
    s_, h, w, wh, ww, sh, sw = 1, 64, 96, 32, 48, 16, 24
    c, m = 128, 64 * 96
    x = rnd(1500, m, c, scale=1.5).to(DEV)
    wq, wk, wv, wm = (rnd(1501 + i, c, c, scale=0.09).to(DEV) for i in range(4))
    norm = torch.nn.LayerNorm(c).to(DEV)
    import ctypes
    f_, r_, k_ = (ctypes.c_int() for _ in range(3))
    ops.lib.um_window_attn_plan(s_, h, w, wh, ww, ctypes.byref(f_), ctypes.byref(r_), ctypes.byref(k_))
    assert (f_.value, r_.value, k_.value) == (0, 48, 4)                   # all key-split, 4 parts
    qp, _, _ = ops.linear_planes(x, (wq,))
    kv, _, n2 = ops.linear_planes(x, (wk, wv))
    ref = ops.window_attention_merge((qp, m, c, 0), (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, wh, ww, sh, sw, 0, wm, norm, x)
    got, cen = _census(lambda: ops.window_attention_qproj_merge(x, wq, (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, wh, ww, sh, sw, 0, wm, norm, x))
    assert cen == {'full': 12 * (48 + 24 + 24 + 12), 'probed': 12 * (24 + 24 + 36), 'probed_then_computed': 0, 'workgroups': 48 * 4}, cen
    assert err(got, ref)[0] < 2e-5
    # mask dominance through a key-split part: a key of another class whose logit beats the row by far more than 100
    idx, label = hp.window_index(h, w, wh, ww, sh, sw)
    win = idx.shape[0] - 1
    a_tok = int(idx[win, 0])
    other = [int(idx[win, j]) for j in range(idx.shape[1]) if label[win, j] != label[win, 0]]
    # crafted through identity projections: q = x2 (Wq = I), k = v = xk (Wk = Wv = I)
    eye = torch.eye(c).to(DEV)
    x2 = rnd(1510, m, c).to(DEV)
    x2[:, 0] = 0.0
    x2[a_tok] = 0.0
    x2[a_tok, 0] = 60.0
    xk = x2.clone()
    xk[a_tok, 0] = 0.0                                                     # (the query's own key must not carry the spike)
    xk[other[-1], 0] = 60.0                                                # q = x2 (Wq = I), k = xk (Wk = I): logit 3600 / sqrt(128) = 318
    qp2, _, _ = ops.linear_planes(x2, (eye,))
    kv2, _, n22 = ops.linear_planes(xk, (eye, eye))
    ref2 = ops.window_attention_merge((qp2, m, c, 0), (kv2, m, n22, 0), (kv2, m, n22, c), s_, h, w, wh, ww, sh, sw, 0, wm, norm, x2)
    got2, cen2 = _census(lambda: ops.window_attention_qproj_merge(x2, eye, (kv2, m, n22, 0), (kv2, m, n22, c), s_, h, w, wh, ww, sh, sw, 0, wm, norm, x2))
    assert cen2['probed_then_computed'] >= 1, cen2
    assert err(got2, ref2)[0] < 2e-5
    want = hp.window_attention(x2.double().cpu()[None], xk.double().cpu()[None], xk.double().cpu()[None], h, w, wh, ww, sh, sw)
    assert (want[0, a_tok] - xk[other[-1]].double().cpu()).abs().max() < 1e-6   # the oracle agrees that the masked key dominates


def test_fused_layer_matches_unfused_layer(ops, golden):
    """The whole FeatureTransformer through the fused tail vs the oracle (fp64) on the golden inputs."""
    g = golden('transformer')
    proto = UniMatch().transformer
    sd = synth_state_dict({k: v.shape for k, v in proto.state_dict().items()}, seed=7)
    proto.load_state_dict(sd)
    proto = proto.to(DEV)
    from unimatch_amd.model import _to_tokens, _to_map
    for attn_type, k in (('swin', 2), ('self_swin2d_cross_swin1d', 4)):
        tag = f'{attn_type}_k{k}'
        f0, f1 = g[f'{tag}.f0'], g[f'{tag}.f1']
        h, w = f0.shape[-2:]
        o0, o1 = proto(ops, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, k)
        two = HipOps('exact')
        two.fused_ffn = False                     # the two-launch FFN stays covered
        two.fused_merge = False                   # ... and merge + LayerNorm as its own launch (and q | k | v planes)
        t0, _ = proto(two, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, k)
        assert err(o0, t0)[0] < 2e-4, tag
        want0, want1 = hp.feature_transformer(f0.double(), f1.double(), {kk: v.double() for kk, v in sd.items()},
                                              attn_type, k)
        assert err(_to_map(o0, h, w), want0)[0] < 2e-4, tag
        assert err(_to_map(o1, h, w), want1)[0] < 2e-4, tag
        assert err(_to_map(o0, h, w), g[f'{tag}.o0'])[0] < 4e-4, tag
        # round 4: both layers' k | v projections of a block as ONE launch (um_kv4_fwd, blocked planes) against the two
        # um_linear_fwd launches it replaces: the same products summed in another order
        per_layer = HipOps('exact')
        per_layer.block_kv = False
        p0, p1 = proto(per_layer, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, k)
        assert err(p0, o0)[0] < 5e-5 and err(p0, o0)[1] < 2e-6 and err(p1, o1)[1] < 2e-6, (tag, err(p0, o0), err(p1, o1))
        # ... and as the previous block's FFN epilogue (um_ffn_kv_fwd, the default) against the stand-alone launch per block: bitwise
        standalone = HipOps('exact')
        standalone.fused_kv = False
        s0, s1 = proto(standalone, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, k)
        assert torch.equal(s0, o0) and torch.equal(s1, o1), tag


@pytest.mark.parametrize('m', [1000, 313 * 128, 313 * 128 + 40])
def test_ffn_with_the_next_blocks_kv_projection(m):
    """um_ffn_kv_fwd: the FFN of block i and the k | v projections of block i + 1 from one launch (the normalised tile goes from the
    LayerNorm straight into kv4_project) -- BITWISE equal to um_ffn_ws_fwd followed by um_kv4_fwd on its result (same fp32 values,
    same hi | lo split, same chunk and product order), in both operand precisions; m = 1000 takes the hidden-split FFN + a second
    launch inside the call, the others the fused tile kernel (census), the last with a partly empty tile."""
    from unimatch_amd import _abi
    lib = _abi.load()
    c = 128
    x, y = rnd(1400, m, c, scale=1.5).to(DEV), rnd(1401, m, c, scale=1.5).to(DEV)
    w1, w2 = rnd(1402, 1024, 256, scale=0.08).to(DEV), rnd(1403, 128, 1024, scale=0.06).to(DEV)
    ws = tuple(rnd(1410 + i, 128, 128, scale=0.09).to(DEV) for i in range(4))
    norm = torch.nn.LayerNorm(c).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * rnd(1404, c).to(DEV))
        norm.bias.copy_(0.1 * rnd(1405, c).to(DEV))
    for prec in ('exact', 'fast'):
        o = HipOps(prec)
        want = o.ffn_ln(x, y, w1, w2, norm)
        want_kv = o.kv4_planes(want, ws)
        lib.um_census_enable(1)
        got, kv = o.ffn_ln_kv(x, y, w1, w2, norm, ws)
        census = _abi.census(lib)
        lib.um_census_enable(0)
        assert (census['ffn_hsplit'] == 1) == (m == 1000) and census['ffn_tile'] + census['ffn_hsplit'] == 1, census
        assert torch.equal(got, want), (prec, err(got, want))
        assert torch.equal(kv, want_kv), prec
    # and against fp64 (exact mode): LayerNorm(W2 gelu(W1 [x | y])) + x, then the four projections
    o = HipOps('exact')
    got, kv = o.ffn_ln_kv(x, y, w1, w2, norm, ws)
    hid = torch.nn.functional.gelu(torch.cat([x, y], 1).double() @ w1.double().t())
    t64 = torch.nn.functional.layer_norm(hid @ w2.double().t(), (c,), norm.weight.double(), norm.bias.double(), norm.eps) + x.double()
    assert err(got, t64)[1] < 2e-6
    planes = kv.view(torch.float16).view(2, 4, m, 128).double().sum(0)
    for j in range(4):
        assert err(planes[j], t64 @ ws[j].double().t())[1] < 4e-6, j


@pytest.mark.parametrize('m', [128, 1000, 2 * 6144 + 40])
def test_kv4_projection(m):
    """um_kv4_fwd: the four k | v projections of a block (transformer.py:58-60) in one launch, blocked operand planes
    [NS][4][M][128] -- against fp64 (hi + lo planes recombined: the split keeps 22 bits) and against um_linear_fwd's planes of the
    same projections; ragged M (last tile partly empty) included; bf16 mode against its own rounding."""
    xs = rnd(1300 + m, m, 128, scale=1.7).to(DEV)
    ws = [rnd(1310 + i, 128, 128, scale=0.09).to(DEV) for i in range(4)]
    want = [(xs.double() @ w.double().t()) for w in ws]
    for prec, tol in (('exact', 3e-6), ('fast', 2e-2)):
        o = HipOps(prec)
        ns = o.nplanes
        kv = o.kv4_planes(xs, tuple(ws))
        halves = kv.view(torch.float16 if prec == 'exact' else torch.bfloat16).view(ns, 4, m, 128)
        got = halves.double().sum(0)                                           # hi + lo
        for j in range(4):
            e_max, e_mean = err(got[j], want[j])
            assert e_mean < tol * 4 and e_max < tol * 40, (prec, j, e_mean, e_max)
        ref, _, n2 = o.linear_planes(xs, (ws[0], ws[3]))                       # the unfused kernel's planes of two of them
        refp = ref.view(halves.dtype).view(ns, m, 256).double().sum(0)
        assert err(got[0], refp[:, :128])[0] < tol * 40 and err(got[3], refp[:, 128:])[0] < tol * 40
        (ks, vs), (kc, vc) = o.kv4_slices(kv, m)
        assert ks[3] == 0 and vs[3] == m * 128 and kc[3] == 2 * m * 128 and vc[3] == 3 * m * 128 and ks[4] == 4 * m * 128


@pytest.mark.parametrize('hw', [(24, 36), (64, 96), (256, 384), (400, 320)])
def test_fused_instance_norm(ops, hw):
    """(400, 320) exceeds the register-resident variant (24 float4 x 1024 threads) and takes the streaming kernel."""
    x = rnd(80, 2, 3, *hw, scale=3.0) + 1.5
    sc = rnd(81, 2, 3, *hw)
    want = torch.nn.functional.instance_norm(x.double())
    assert err(ops.instance_norm(x.to(DEV), relu=False), want)[0] < 2e-6
    assert err(ops.instance_norm(x.to(DEV), relu=True), want.clamp(min=0))[0] < 2e-6
    got = ops.instance_norm(x.to(DEV), relu=True, shortcut=sc.to(DEV))
    assert err(got, (want.clamp(min=0) + sc.double()).clamp(min=0))[0] < 2e-6


def test_hip_graph_replay_matches_eager():
    """Whole forward captured into a HIP graph: bitwise equal to the eager result, also after new inputs."""
    from unimatch_amd.graph import GraphedUniMatch
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}))
    model = model.to(DEV)
    graphed = GraphedUniMatch(model)
    for seed in (5, 6):
        i0, i1 = synth_images(2, 64, 96, seed=seed, kind='shift')
        i0, i1 = i0.to(DEV), i1.to(DEV)
        want = model(i0, i1, **fk)['flow_preds'][0]
        got = graphed(i0, i1, **fk)['flow_preds'][0]
        assert torch.equal(got, want)
    assert len(graphed._graphs) == 1 and all(v is not False for v in graphed._graphs.values())


@pytest.mark.parametrize('cfg', [(8, 2, False), (4, 2, False), (8, 1, True), (4, 1, False)])
def test_convex_upsample(ops, cfg):
    factor, v, is_depth = cfg
    b, h, w = 2, 12, 20
    flow = rnd(90, b, v, h, w, scale=5.0)
    mask = rnd(91, b, 9 * factor * factor, h, w, scale=2.0)
    want = om.convex_upsample(flow.double(), mask.double(), factor, is_depth=is_depth)
    got = ops.convex_upsample(flow.to(DEV), mask.to(DEV), factor, is_depth)
    assert got.shape == want.shape and err(got, want)[0] < 2e-6 * max(1.0, want.abs().max().item())
    # the same mask in channels-last layout (what um_conv2d_fwd produces): bitwise the same result
    nhwc = mask.permute(0, 2, 3, 1).reshape(b * h * w, -1).contiguous().to(DEV)
    assert torch.equal(ops.convex_upsample(flow.to(DEV), nhwc, factor, is_depth, mask_nhwc=True), got)


def test_weight_range_is_checked(ops):
    """Exact mode stores weights as fp16 planes of w * 2^10: a weight of 64 or more cannot be represented and must be refused
    when its planes are built, not turned into inf / NaN outputs."""
    w = torch.full((128, 128), 0.01, device=DEV)
    ops.weight_planes((w,))                                        # fine
    bad = w.clone()
    bad[3, 5] = 70.0
    with pytest.raises(ValueError, match='does not fit the fp16 operand planes'):
        ops.weight_planes((bad,))


@pytest.mark.parametrize('kind', ['smooth', 'noisy', 'mixed', 'border'])
def test_cost_volume_matrix_core_path(ops, kind):
    """um_local_corr_with_flow_feat: 8 x 4 pixel tiles with coherent flow go through the matrix cores (one 32 x 32 x 128 product
    per window row, split-fp16 operands), the others through the pixel-at-a-time path of the same kernel.  Against the fp64
    oracle (matching.py:86-123 restated), against the same kernel with every tile forced onto the VALU path, and both output
    forms.  'border': flows that push whole windows out of the image (zeros padding) and exactly integer flows."""
    b, h, w = 2, 32, 48
    f0, f1 = rnd(130, b, C, h, w), rnd(131, b, C, h, w)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    smooth = torch.stack([2.3 * torch.sin(yy / 5.0) + 0.05 * xx, 1.7 * torch.cos(xx / 7.0) - 0.5], 0)[None].repeat(b, 1, 1, 1).float()
    if kind == 'smooth':
        flow = smooth
    elif kind == 'noisy':
        flow = rnd(132, b, 2, h, w, scale=9.0)
    elif kind == 'mixed':
        flow = smooth.clone()
        flow[:, :, :, 24:] += rnd(133, b, 2, h, 24, scale=12.0)           # right half incoherent
        flow[:, :, 8:12, :8] += 3.1                                       # a coherent tile with a different motion
    else:
        flow = smooth.clone()
        flow[0, 0] += 45.0                                                # image 0: everything samples right of the image
        flow[1] = torch.round(flow[1])                                    # image 1: integer flows (weights 1, 0, 0, 0)
        flow[1, 1, :6] -= 7.0                                             # top rows sample above the image
    flow = flow.contiguous()
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    want = hp.local_corr_with_flow(f0.double(), f1.double(), flow.double(), 4)
    assert ops._k4_feat_planes(t0, t1, h, w, 4) is not None               # the matrix-core entry point serves this geometry
    got = ops.local_corr_with_flow(t0, t1, flow.to(DEV), h, w, 4)
    scale = max(1.0, want.abs().max().item())
    assert err(got, want)[1] < 3e-6 * scale, (kind, err(got, want))
    ops.k4_flags = 1
    try:
        valu = ops.local_corr_with_flow(t0, t1, flow.to(DEV), h, w, 4)
    finally:
        ops.k4_flags = 0
    assert err(valu, want)[1] < 3e-6 * scale
    rows = b * h * w
    buf = ops.planes_buffer(rows, 96)
    ops.local_corr_with_flow_planes(t0, t1, flow.to(DEV), h, w, 4, buf, 96)
    pl = buf.view(torch.float16).view(2, rows + 1, 96).float()
    back = pl.sum(0)[:rows, :81].view(b, h, w, 81).permute(0, 3, 1, 2)
    assert (back - got).abs().max().item() < 2e-6 * scale
    assert torch.equal(pl[:, :rows, 81:], torch.zeros(2, rows, 15, device=DEV))
    assert torch.equal(pl[:, rows], torch.zeros(2, 96, device=DEV))


def test_cost_volume_dispatch_is_a_pure_function_of_the_call():
    """Which kernel serves the cost volume depends on the call's geometry only (radius 4 on whole 8 x 4 tiles: k4m_kernel, whose
    per-tile product / gather choice depends on the flow values only) -- never on earlier calls or on timing (round 2 routed by
    an asynchronously read counter).  Interleaving coherent and incoherent launches in any order gives bitwise-equal results
    for equal inputs, and the launch census shows the same kernel every time."""
    from unimatch_amd import _abi
    o = HipOps('exact')
    lib = _abi.load()
    b, h, w = 1, 32, 48
    f0, f1 = rnd(150, b, C, h, w), rnd(151, b, C, h, w)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    noisy = rnd(152, b, 2, h, w, scale=20.0).to(DEV)
    smooth = torch.full((b, 2, h, w), 1.3, device=DEV)
    want = {id(noisy): hp.local_corr_with_flow(f0.double(), f1.double(), noisy.cpu().double(), 4),
            id(smooth): hp.local_corr_with_flow(f0.double(), f1.double(), smooth.cpu().double(), 4)}
    lib.um_census_enable(1)
    first = {}
    for flow in (noisy, noisy, smooth, noisy, smooth, smooth, noisy, noisy, noisy, smooth):
        got = o.local_corr_with_flow(t0, t1, flow, h, w, 4)
        assert err(got, want[id(flow)])[1] < 3e-6 * max(1.0, want[id(flow)].abs().max().item())
        if id(flow) in first:
            assert torch.equal(got, first[id(flow)])
        first[id(flow)] = got
    census = _abi.census(lib)
    lib.um_census_enable(0)
    assert census['k4_mfma'] == 10 and census['k4_valu'] == 0
    # round 5: incoherent flow is served TARGET-ORDERED (pixels grouped by the cell of f1 they sample: every group shares one window
    # and runs on the matrix cores).  Switched off (flags bit 1: natural tiles, pixel path) the same call must agree to rounding --
    # and with flows that leave the map entirely the groups that sample nothing must write exact zeros either way.
    o.k4_flags = 2
    try:
        natural = o.local_corr_with_flow(t0, t1, noisy, h, w, 4)
    finally:
        o.k4_flags = 0
    scale = max(1.0, want[id(noisy)].abs().max().item())
    assert err(natural, want[id(noisy)])[1] < 3e-6 * scale and err(natural, first[id(noisy)])[0] < 3e-6 * scale
    away = noisy.clone()
    away[:, 0, :, : w // 2] += 500.0                                           # left half samples far right of the image
    got_away = o.local_corr_with_flow(t0, t1, away, h, w, 4)
    assert torch.equal(got_away[:, :, :, : w // 2], torch.zeros_like(got_away[:, :, :, : w // 2]))
    assert torch.equal(got_away[:, :, :, w // 2:], first[id(noisy)][:, :, :, w // 2:])      # the other pixels: bitwise as before
    # a geometry the matrix-core kernel does not serve (width not a multiple of 8) always takes the VALU kernel
    lib.um_census_enable(1)
    f0b, f1b = rnd(153, 1, C, 12, 20), rnd(154, 1, C, 12, 20)
    o.local_corr_with_flow(tok(f0b).to(DEV), tok(f1b).to(DEV), rnd(155, 1, 2, 12, 20, scale=3.0).to(DEV), 12, 20, 4)
    assert _abi.census(lib)['k4_valu'] == 1 and _abi.census(lib)['k4_mfma'] == 0
    lib.um_census_enable(0)


def test_cost_volume_target_order_at_full_size():
    """The target-ordered cost volume at config 3's refinement geometry (4 x 128 x 240: 32 sorting workgroups, more (image, cell) groups
    than a workgroup has threads, spans that end inside an image): against the natural-tile walk of the same call (flags bit 1; that
    path is pinned to the oracle at small sizes above) to rounding, bitwise reproducible, exact zeros where nothing is sampled, and
    bitwise independent of what shares a pixel's group (the other images' flow changed)."""
    o = HipOps('exact')
    b, h, w = 4, 128, 240
    g = torch.Generator().manual_seed(160)
    t0 = (torch.randn(b, h * w, C, generator=g) * 0.5).to(DEV)
    t1 = (torch.randn(b, h * w, C, generator=g) * 0.5).to(DEV)
    flow = (torch.randn(b, 2, h, w, generator=g) * 30.0).to(DEV)
    flow[1, 0, :, : w // 3] += 900.0                                          # a third of image 1 samples nothing
    flow[2] = 0.7                                                            # image 2 is coherent (its pixels still go through the sort)
    got = o.local_corr_with_flow(t0, t1, flow, h, w, 4)
    again = o.local_corr_with_flow(t0, t1, flow, h, w, 4)
    assert torch.isfinite(got).all() and torch.equal(got, again)
    o.k4_flags = 2
    try:
        natural = o.local_corr_with_flow(t0, t1, flow, h, w, 4)
    finally:
        o.k4_flags = 0
    scale = max(1.0, natural.abs().max().item())
    assert (got - natural).abs().max().item() < 3e-6 * scale
    assert torch.equal(got[1, :, :, : w // 3], torch.zeros_like(got[1, :, :, : w // 3]))
    # oracle leg at full size: images 0 (incoherent flow) and 1 (a third samples nothing) of the SORTED result
    # against matching.py:86-123 evaluated in fp64 on the CPU
    for img in (0, 1):
        f0 = t0[img:img + 1].cpu().double().transpose(1, 2).reshape(1, C, h, w)
        f1 = t1[img:img + 1].cpu().double().transpose(1, 2).reshape(1, C, h, w)
        want = hp.local_corr_with_flow(f0, f1, flow[img:img + 1].cpu().double(), 4)
        mx, mean = err(got[img:img + 1], want)
        assert mean < 3e-6 * max(1.0, want.abs().max().item()) and mx < 3e-5 * max(1.0, want.abs().max().item()), (img, mx, mean)
    other = flow.clone()
    other[0] = torch.randn(2, h, w, generator=g).to(DEV) * 30.0               # different groups everywhere in image 0 ...
    got2 = o.local_corr_with_flow(t0, t1, other, h, w, 4)
    assert torch.equal(got2[1:], got[1:])                                    # ... the other images do not notice


def test_concurrent_forwards_on_two_streams():
    """``ConcurrentUniMatch``: a batch as two forwards on two HIP streams.  Every part is bitwise the plain forward of its samples; against
    the one-forward result the difference stays at the fp32 noise floor (launch-size dependent summation orders only); repeated calls are
    bitwise equal (no race on the caches the first, sequential, call builds); the refinement path (plane buffers per stream) included."""
    from unimatch_amd.streams import ConcurrentUniMatch
    for name, b, hh, ww in (('gmflow_s1', 4, 128, 192), ('gmflow_s2_rr6', 3, 128, 192), ('gmdepth_s1', 4, 96, 128)):
        ck, fk = CONFIGS[name]
        model = UniMatch(**ck).eval()
        model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
        model = model.to(DEV)
        i0, i1 = synth_images(b, hh, ww, seed=31, kind='shift', normalized=(fk['task'] != 'flow'))
        i0, i1 = i0.to(DEV), i1.to(DEV)
        kw = dict(fk)
        if fk['task'] == 'depth':
            k, pose = synth_camera(b, hh, ww)
            kw.update(intrinsics=k.to(DEV), pose=pose.to(DEV))
        whole = model(i0, i1, **kw)['flow_preds'][0]
        wrapped = ConcurrentUniMatch(model, parts=2)
        first = wrapped(i0, i1, **kw)['flow_preds'][0]                # sequential: builds the caches
        runs = [wrapped(i0, i1, **kw)['flow_preds'][0] for _ in range(4)]      # concurrent
        torch.cuda.synchronize()
        assert all(torch.equal(r, first) for r in runs)
        lo = 0
        for r, n in enumerate((b - b // 2, b // 2)):
            pk = dict(kw)
            for key in ('intrinsics', 'pose'):
                if pk.get(key) is not None:
                    pk[key] = pk[key][lo:lo + n].contiguous()
            alone = model(i0[lo:lo + n].contiguous(), i1[lo:lo + n].contiguous(), **pk)['flow_preds'][0]
            assert torch.equal(first[lo:lo + n], alone)
            lo += n
        assert torch.isfinite(first).all()
        assert (first - whole).abs().max().item() < 1e-3 * max(1.0, whole.abs().max().item())
        if name == 'gmflow_s1':
            # a new backend (other precision: every shared cache entry is rebuilt) sends the next forward through the sequential path
            # again; the concurrent ones after it are bitwise that result
            model.set_precision('fast')
            fast_first = wrapped(i0, i1, **kw)['flow_preds'][0]
            assert wrapped._backend[1] is not None and wrapped._backend[0] == id(model.ops)
            fast_runs = [wrapped(i0, i1, **kw)['flow_preds'][0] for _ in range(3)]
            torch.cuda.synchronize()
            assert all(torch.equal(r, fast_first) for r in fast_runs)
            gen = model.ops.cache_generation
            model.invalidate_weights()
            assert model.ops.cache_generation > gen
            again = wrapped(i0, i1, **kw)['flow_preds'][0]            # sequential (the state of the backend changed), rebuilds
            assert torch.equal(again, fast_first)
            model.set_precision('exact')


def _refine_model(name, gain=0.02):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=gain))
    return model.to(DEV), fk


@pytest.mark.parametrize('name', ['gmflow_s2_rr6', 'gmstereo_s2_rr3'])
def test_refinement_configs_are_run_to_run_reproducible(name):
    """Two forwards of a two-scale + refinement config on the same inputs are BITWISE equal, and so is a third one from a fresh
    module (no state carried on HipOps between forwards decides anything): config 3 / 4 outputs are reproducible."""
    model, fk = _refine_model(name, gain=1.0)                           # random init: incoherent scale-1 flow, the case that flipped
    i0, i1 = synth_images(2, 128, 192, seed=77, kind='shift', normalized=(fk['task'] != 'flow'))
    i0, i1 = i0.to(DEV), i1.to(DEV)
    a = model(i0, i1, **fk)['flow_preds'][0]
    b = model(i0, i1, **fk)['flow_preds'][0]
    model2, _ = _refine_model(name, gain=1.0)
    c = model2(i0, i1, **fk)['flow_preds'][0]
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_hip_graph_replay_matches_eager_with_refinement():
    """HIP-graph capture of a refinement config (cost volume x 6 inside the GRU loop): replay is bitwise equal to eager, on the
    captured inputs and on new ones (nothing about the cost-volume dispatch is frozen into the graph)."""
    from unimatch_amd.graph import GraphedUniMatch
    model, fk = _refine_model('gmflow_s2_rr6')
    graphed = GraphedUniMatch(model)
    for seed in (15, 16, 17):
        i0, i1 = synth_images(1, 128, 192, seed=seed, kind='shift' if seed != 17 else 'noise')
        i0, i1 = i0.to(DEV), i1.to(DEV)
        want = model(i0, i1, **fk)['flow_preds'][0]
        got = graphed(i0, i1, **fk)['flow_preds'][0]
        assert torch.equal(got, want), seed
    assert len(graphed._graphs) == 1 and all(v is not False for v in graphed._graphs.values())


def test_local_corr_softmax_matrix_core_path(ops):
    """um_local_corr_softmax_mfma (matching.py:39-83 on the cost-volume kernel's product path: every tile coherent) against the
    fp64 oracle and against the VALU kernel, incl. the image border (out-of-image taps take part with logit -1e9)."""
    b, h, w = 2, 32, 48
    for sc in (1.0, 3.0):                                             # soft and peaky softmaxes
        f0, f1 = rnd(140, b, C, h, w, scale=sc), rnd(141, b, C, h, w, scale=sc)
        f1 = 0.6 * f0.roll((1, -2), (2, 3)) + 0.4 * f1
        t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
        want = hp.local_corr_softmax(f0.double(), f1.double(), 4)
        assert ops.k4_mfma and ops.lib.um_local_corr_with_flow_feat_supported(h, w, C, 4)
        got = ops.local_corr_softmax(t0, t1, h, w, 4)
        ops.k4_mfma = False
        try:
            valu = ops.local_corr_softmax(t0, t1, h, w, 4)
        finally:
            ops.k4_mfma = True
        assert err(got, want)[1] < 2e-5 and err(valu, want)[1] < 2e-5, (sc, err(got, want), err(valu, want))


# ------------------------------------------------------------------ small-launch hand-offs under load; RCCL at world size 1
def test_split_handoffs_repeat_under_uneven_load():
    """The key-split attention and hidden-split FFN launches hand partial results from workgroup to workgroup through memory
    (agent-scope accesses + a flag, workspace left zero by every launch).  A race there would be intermittent, so: > 200
    launches per kernel at the batch-1 geometries, each compared BITWISE with the first (the merge order is fixed), while a
    second stream keeps the memory system unevenly busy; the census proves the split instantiations ran and the hand-off
    FLAGS (the head of each workspace; the slots behind them keep stale partials, which is fine) must be zero afterwards."""
    from unimatch_amd import _abi
    o = HipOps('exact')
    lib = _abi.load()
    c = 128
    side = torch.cuda.Stream()
    big = torch.empty(64 << 20, dtype=torch.float32, device=DEV)              # 256 MB: streaming traffic on the side stream
    norm = torch.nn.LayerNorm(c).to(DEV)
    lib.um_census_enable(1)
    launches = 0
    for gi, (s_, h, w, wh, ww, sh, sw, rot) in enumerate([(1, 32, 48, 32, 48, 0, 0, 0), (2, 40, 56, 20, 28, 10, 14, 1),
                                                          (1, 64, 96, 32, 48, 16, 24, 0), (2, 32, 48, 16, 24, 8, 12, 1)]):
        m = s_ * h * w
        x = rnd(700 + gi, m, c, scale=1.5).to(DEV)
        xt = rnd(710 + gi, m, c, scale=1.5).to(DEV)
        wq, wk, wv, wm = (rnd(720 + 4 * gi + i, c, c, scale=0.09).to(DEV) for i in range(4))
        kv, _, n2 = o.linear_planes(xt, (wk, wv))
        ref = None
        for it in range(55):
            if it % 3 != 2:                                                   # two launches under load, one on a quiet chip
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    big.mul_(1.0001) if it % 2 else big[: big.numel() // 2].copy_(big[big.numel() // 2:])
            got = o.window_attention_qproj_merge(x, wq, (kv, m, n2, 0), (kv, m, n2, c), s_, h, w, wh, ww, sh, sw, rot, wm, norm, x)
            launches += 1
            if ref is None:
                ref = got
                assert torch.isfinite(ref).all()
            else:
                assert torch.equal(got, ref), (gi, it)
    census = _abi.census(lib)
    assert census['wattn_ksplit'] == launches >= 200 and census['wattn_tile'] == 0, census
    w1 = rnd(740, 1024, 256, scale=0.08).to(DEV)
    w2 = rnd(741, 128, 1024, scale=0.06).to(DEV)
    launches = 0
    for gi, m in enumerate([2 * 2240, 2 * 6144, 2 * 4800, 1000]):
        x, y = rnd(750 + gi, m, c, scale=1.5).to(DEV), rnd(760 + gi, m, c, scale=1.5).to(DEV)
        ref = None
        for it in range(55):
            if it % 3 != 2:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    big.mul_(1.0001) if it % 2 else big[: big.numel() // 2].copy_(big[big.numel() // 2:])
            got = o.ffn_ln(x, y, w1, w2, norm)
            launches += 1
            if ref is None:
                ref = got
                assert torch.isfinite(ref).all()
            else:
                assert torch.equal(got, ref), (gi, it)
    census = _abi.census(lib)
    lib.um_census_enable(0)
    assert census['ffn_hsplit'] == launches >= 200 and census['ffn_tile'] == 0, census
    torch.cuda.synchronize()
    assert {k.kind for k, _ in o.workspace_entries()} == {'attn_ksplit', 'ffn_hsplit'}
    for key, buf in o.workspace_entries():
        assert int(buf[:64].count_nonzero()) == 0, key                       # the flags every launch must leave zero (>= 16 of them)


def _graph_case(name, hh, ww, batch=1):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}))
    model = model.to(DEV)
    i0, i1 = synth_images(batch, hh, ww, seed=11, kind='shift')
    return model, i0.to(DEV), i1.to(DEV), fk


def test_graph_capture_owns_its_split_workspaces():
    """the split workspaces (arrival counters) of a captured forward are allocated and zeroed by the eager
    warm-up, never inside the capture; every graph owns its own buffers (two graphs share no counter) and the eager path keeps
    its per-stream ones; a first-time request inside a capture is refused instead of baking in a pool buffer."""
    from unimatch_amd.graph import GraphedUniMatch
    model, i0, i1, fk = _graph_case('gmflow_s1', 320, 448)        # config 1's size: key-split attention, hidden-split FFN
    eager = model(i0, i1, **fk)['flow_preds'][0]
    ops = model.ops
    entries = lambda: {k for k, _ in ops.workspace_entries()}
    eager_keys = entries()
    assert eager_keys and all(isinstance(k.owner, int) for k in eager_keys)  # keyed by stream
    g1, g2 = GraphedUniMatch(model), GraphedUniMatch(model)
    a = g1(i0, i1, **fk)['flow_preds'][0]
    b = g2(i0, i1, **fk)['flow_preds'][0]
    assert torch.equal(a, eager) and torch.equal(b, eager)
    assert entries() == eager_keys and ops.workspace_scope() == (None, 0)   # nothing of the graphs is left in the shared cache
    w1, w2 = (next(iter(g._graphs.values()))['workspaces'] for g in (g1, g2))
    assert w1 and w2 and {k.kind for k in w1} == {k.kind for k in eager_keys}
    ptrs = [t.data_ptr() for ws in (w1, w2, dict(ops.workspace_entries())) for t in ws.values()]
    assert len(set(ptrs)) == len(ptrs)                                       # every graph and the eager path: separate counters
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()                        # replayed concurrently on two streams, repeatedly
    for _ in range(20):
        for g, st in ((g1, s1), (g2, s2)):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                next(iter(g._graphs.values()))['graph'].replay()
    torch.cuda.synchronize()
    for g in (g1, g2):
        assert torch.equal(next(iter(g._graphs.values()))['out'], eager)
    for ws in (w1, w2):
        for key, buf in ws.items():
            if isinstance(key.kind, str):                                    # the counters (not the refinement's plane buffers)
                assert int(buf[:64].count_nonzero()) == 0
    # first-time request inside a capture (a user's own torch.cuda.graph, no warm-up under an owner): a capture-private zeroed
    # buffer that is NOT cached -- no later launch can meet counters an aborted capture left behind (raising here
    # turned such captures into a permanent eager fallback)
    fresh = HipOps('exact')
    graph = torch.cuda.CUDAGraph()
    x = rnd(900, 2240, 128).to(DEV)
    with torch.cuda.graph(graph):
        ws = fresh._split_workspace('ffn_hsplit', (x.shape[0], 1024), x.device)      # config 1's FFN: a hidden-split launch
        probe = ws[:64].clone()
    graph.replay()
    torch.cuda.synchronize()
    assert int(probe.count_nonzero()) == 0 and not fresh.workspace_entries()
    # a graph around a WRAPPER of the model (ShardedUniMatch at world size 1) finds the HipOps through it: its workspaces are
    # owned by the graph exactly as above, and the capture succeeds (no eager fallback)
    from unimatch_amd.dist import ShardedUniMatch
    g3 = GraphedUniMatch(ShardedUniMatch(model, rank=0, world=1))
    c = g3(i0, i1, **fk)['flow_preds'][0]
    entry = next(iter(g3._graphs.values()))
    assert entry is not False and entry['workspaces'] and torch.equal(c, eager)
    assert entries() == eager_keys and ops.workspace_scope() == (None, 0)


def test_graph_of_a_forward_with_concurrent_parts_owns_one_workspace_set_per_part():
    """a captured forward whose batch runs as two concurrent parts (UniMatch.forward's own plan, or forced) must
    not share arrival counters / partial buffers / activation planes between the parts: owned buffers are keyed by (graph token,
    part).  Small launches (key-split attention, hidden-split FFN) + the refinement's plane buffers; replay bitwise = eager."""
    from unimatch_amd.graph import GraphedUniMatch
    from unimatch_amd.streams import ConcurrentUniMatch
    model, fk = _refine_model('gmflow_s2_rr6')
    i0, i1 = synth_images(2, 128, 192, seed=21, kind='shift')
    i0, i1 = i0.to(DEV), i1.to(DEV)
    model.launch_parts = 2
    try:
        eager = model(i0, i1, **fk)['flow_preds'][0]                 # sequential first call
        eager2 = model(i0, i1, **fk)['flow_preds'][0]                # concurrent
        assert torch.equal(eager, eager2)
        for wrap in (lambda m: m, lambda m: ConcurrentUniMatch(m, parts=2)):
            graphed = GraphedUniMatch(wrap(model))
            got = graphed(i0, i1, **fk)['flow_preds'][0]
            entry = next(iter(graphed._graphs.values()))
            assert entry is not False and torch.equal(got, eager)
            lanes = {k.owner[1] for k in entry['workspaces']}
            assert lanes == {0, 1}, lanes
            by_lane = {ln: {(k.kind, k.geometry): t.data_ptr() for k, t in entry['workspaces'].items() if k.owner[1] == ln}
                       for ln in lanes}
            assert set(by_lane[0]) == set(by_lane[1])
            assert all(by_lane[0][name] != by_lane[1][name] for name in by_lane[0])
            for _ in range(10):
                again = graphed(i0, i1, **fk)['flow_preds'][0]
            torch.cuda.synchronize()
            assert torch.equal(again, eager)
            assert model.ops.workspace_scope() == (None, 0)
    finally:
        model.launch_parts = None


def test_small_launch_workspaces_survive_a_change_of_geometry():
    """Round 6 regression: the split small-launch workspaces (key-split attention, hidden-split FFN) keep their arrival counters at the
    head of the buffer, `tiles` of them -- a buffer left by ANOTHER geometry has that geometry's partial results where this launch's
    counters must be zero.  One model, batch 1: 512x768, then 320x448, then 512x768 again must reproduce the first result bitwise (it
    produced non-finite values); and a batch of 3 as parts of 2 + 1 pairs (three geometries through one stream in the sequential first
    call) equals the forwards of its parts."""
    model, i0, i1, fk = _graph_case('gmflow_s1', 512, 768, batch=3)
    j0, j1 = synth_images(1, 320, 448, seed=12, kind='shift')
    j0, j1 = j0.to(DEV), j1.to(DEV)
    a = model(i0[:1], i1[:1], **fk)['flow_preds'][0]
    b = model(j0, j1, **fk)['flow_preds'][0]
    a2 = model(i0[:1], i1[:1], **fk)['flow_preds'][0]
    b2 = model(j0, j1, **fk)['flow_preds'][0]
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.equal(a, a2) and torch.equal(b, b2)
    two = model(i0[:2], i1[:2], **fk)['flow_preds'][0]
    one = model(i0[2:], i1[2:], **fk)['flow_preds'][0]
    model.launch_parts = 2
    try:
        first = model(i0, i1, **fk)['flow_preds'][0]                 # sequential: 2 pairs, then 1 pair, on one stream
        again = [model(i0, i1, **fk)['flow_preds'][0] for _ in range(4)]     # concurrent
    finally:
        model.launch_parts = None
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and torch.equal(first, torch.cat([two, one], 0))
    assert all(torch.equal(r, first) for r in again)
    # two geometries whose workspaces have EQUAL byte counts but different plans -- attention: 32 query tiles in 4 key parts
    # against 64 tiles in 2; FFN: 448 against 480 rows in 4 tiles -- get a buffer each, and alternating them stays bitwise
    lib, ops = model.ops.lib, model.ops
    cases = (('attn_ksplit', (1, 128, 992), (2, 128, 800), (2, 16, 124, 8, 62), (4, 16, 100, 8, 50)),
             ('ffn_hsplit', (1, 64, 224), (1, 96, 160), (448, 1024), (480, 1024)))
    for kind, img_a, img_b, geo_a, geo_b in cases:
        size = lib.um_window_attn_ksplit_workspace_bytes if kind == 'attn_ksplit' else lib.um_ffn_split_workspace_bytes
        assert size(*geo_a) == size(*geo_b) > 0
        pa, pb = (tuple(t.to(DEV) for t in synth_images(*g, seed=14, kind='shift')) for g in (img_a, img_b))
        ra, rb = (model(*p, **fk)['flow_preds'][0] for p in (pa, pb))
        ra2, rb2 = (model(*p, **fk)['flow_preds'][0] for p in (pa, pb))
        assert torch.isfinite(ra).all() and torch.isfinite(rb).all() and torch.equal(ra, ra2) and torch.equal(rb, rb2), kind
        bufs = {k.geometry: buf for k, buf in ops.workspace_entries() if k.kind == kind}
        assert bufs[geo_a].data_ptr() != bufs[geo_b].data_ptr(), kind
    model.check_operand_range()


def test_a_part_that_raises_leaves_the_model_usable(monkeypatch):
    """the concurrent fork / join is exception-safe.  With two parts forced, a side part that raises propagates its error,
    leaves no workspace scope behind and the caller's stream joined with the side stream: the next plain call is bitwise the warm one."""
    model, i0, i1, fk = _graph_case('gmflow_s1', 128, 192, batch=2)
    model.launch_parts = 2
    try:
        warm = model(i0, i1, **fk)['flow_preds'][0]                  # sequential first call
        caller, plain = torch.cuda.current_stream(), model._forward_one

        def side_part_raises(*args, **kw):
            if torch.cuda.current_stream() != caller:
                raise ValueError('side part failed')
            return plain(*args, **kw)

        monkeypatch.setattr(model, '_forward_one', side_part_raises)
        with pytest.raises(ValueError, match='side part failed'):
            model(i0, i1, **fk)                                      # concurrent: part 1 is enqueued first, on the side stream
        assert model.ops.workspace_scope() == (None, 0)
        monkeypatch.undo()
        again = model(i0, i1, **fk)['flow_preds'][0]
    finally:
        model.launch_parts = None
    torch.cuda.synchronize()
    assert torch.equal(again, warm)


@pytest.mark.parametrize('name', ['gmflow_s1', 'gmflow_s2_rr6', 'gmstereo_s2_rr3'])
def test_results_do_not_depend_on_the_history_of_calls(name):
    """One model, a shuffled sequence of batch / frame sizes (one forward and two concurrent parts, whole-tile and split small-launch
    kernels, even and uneven parts), every input visited three times: a result is a function of the input alone -- bitwise equal at every
    visit, whatever ran before it (the stale-workspace bug of round 6 was of this kind), finite, and no operand-range flag."""
    import random
    model, fk = _refine_model(name) if name != 'gmflow_s1' else (_graph_case(name, 64, 96)[0], CONFIGS[name][1])
    cases = [(1, 320, 448), (2, 256, 384), (3, 512, 768), (4, 128, 192), (1, 512, 768), (5, 320, 448), (8, 256, 384), (2, 512, 768), (6, 512, 768)]
    if name != 'gmflow_s1':
        cases = [(1, 256, 384), (2, 256, 384), (3, 384, 512), (4, 256, 384), (2, 128, 192), (5, 256, 256), (3, 256, 384)]
    inputs = {}
    for i, (b, hh, ww) in enumerate(cases):
        i0, i1 = synth_images(b, hh, ww, seed=200 + i, kind='shift', normalized=(fk['task'] != 'flow'))
        inputs[(b, hh, ww)] = (i0.to(DEV), i1.to(DEV))
    order = cases * 3
    random.Random(7).shuffle(order)
    seen = {}
    for key in order:
        out = model(*inputs[key], **fk)['flow_preds'][0]
        assert torch.isfinite(out).all(), key
        if key in seen:
            assert torch.equal(out, seen[key]), key
        else:
            seen[key] = out.clone()
    model.check_operand_range()


def test_two_parts_with_bidirectional_flow_keep_the_reference_layout():
    """pred_bidir_flow doubles the batch inside the model ([forward; backward], unimatch.py:139-141); with the batch cut into parts the
    result must come back in that layout: rows [0, B) the forward flows of samples 0 .. B-1, rows [B, 2B) the backward ones -- bitwise
    the rows of the parts' own forwards, for even and uneven parts."""
    model, _, _, fk = _graph_case('gmflow_s1', 64, 96)
    for b in (4, 3):
        i0, i1 = synth_images(b, 128, 192, seed=33 + b, kind='shift')
        i0, i1 = i0.to(DEV), i1.to(DEV)
        model.launch_parts = 2
        try:
            first = model(i0, i1, pred_bidir_flow=True, **fk)['flow_preds'][0]
            second = model(i0, i1, pred_bidir_flow=True, **fk)['flow_preds'][0]
        finally:
            model.launch_parts = 1
        assert first.shape == (2 * b, 2, 128, 192) and torch.equal(first, second)
        lo = 0
        for n in (b - b // 2, b // 2):
            alone = model(i0[lo:lo + n].contiguous(), i1[lo:lo + n].contiguous(), pred_bidir_flow=True, **fk)['flow_preds'][0]
            assert torch.equal(first[lo:lo + n], alone[:n]) and torch.equal(first[b + lo:b + lo + n], alone[n:])
            lo += n
        model.launch_parts = None


def test_forward_chooses_its_launch_mode_per_call():
    """the number of concurrent forwards is a property of UniMatch.forward, chosen by a pure function of the call
    (streams.forward_parts).  A flow batch of four 512x768 pairs runs as two parts (bitwise the forwards of its halves); the same
    model on two pairs, and a forced launch_parts = 1, run as one forward."""
    from unimatch_amd.streams import forward_parts
    model, i0, i1, fk = _graph_case('gmflow_s1', 512, 768, batch=8)
    assert forward_parts('flow', fk['attn_type'], 1, False, 8, 512, 768) == 2
    assert forward_parts('flow', fk['attn_type'], 1, False, 2, 512, 768) == 1
    first = model(i0, i1, **fk)['flow_preds'][0]
    assert model._runner is not None and len(model._runner._seen) == 1
    second = model(i0, i1, **fk)['flow_preds'][0]                    # concurrent
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    model.launch_parts = 1
    halves = torch.cat([model(i0[:4], i1[:4], **fk)['flow_preds'][0], model(i0[4:], i1[4:], **fk)['flow_preds'][0]], 0)
    model.launch_parts = None
    assert torch.equal(first, halves)
    seen = len(model._runner._seen)
    pair = model(i0[:2], i1[:2], **fk)['flow_preds'][0]              # two pairs: one forward by plan, nothing new in the runner
    assert len(model._runner._seen) == seen and pair.shape[0] == 2
    model.launch_parts = 1
    whole = model(i0, i1, **fk)['flow_preds'][0]
    model.launch_parts = None
    assert torch.isfinite(whole).all() and whole.shape == first.shape
    # one forward of 8 against two of 4: launch-size dependent summation orders only (random init amplifies them: compare medians)
    assert (first - whole).abs().median().item() < 1e-2


def test_sharded_model_through_the_rccl_gather_at_world_one():
    """``ShardedUniMatch`` + HipOps with the gather forced at world size 1: shard -> forward -> ``um_allgather_preds`` (RCCL) ->
    reassembly must return exactly what the plain model returns (flow, and the bidirectional [forward; backward] layout)."""
    from unimatch_amd import dist as umd
    model, i0, i1, fk = _graph_case('gmflow_s1', 64, 96, batch=3)
    want = model(i0, i1, **fk)['flow_preds'][0]
    umd._GATHER = None
    sharded = umd.ShardedUniMatch(model, rank=0, world=1, force_gather=True)
    got = sharded(i0, i1, **fk)['flow_preds'][0]
    assert umd.GATHER_KIND and 'um_allgather_preds' in umd.GATHER_KIND, umd.GATHER_KIND
    assert got.shape == want.shape and torch.equal(got, want)
    want2 = model(i0, i1, pred_bidir_flow=True, **fk)['flow_preds'][0]
    got2 = sharded(i0, i1, pred_bidir_flow=True, **fk)['flow_preds'][0]
    assert got2.shape == want2.shape == (6, 2, 64, 96) and torch.equal(got2, want2)
    umd._GATHER.close()
    umd._GATHER = None


def test_rccl_allgather_at_world_size_one(tmp_path):
    """The library's own collective path (um_comm_unique_id -> um_comm_init_rank -> um_allgather_preds = ncclAllGather, RCCL
    bound by dlopen) at world size 1, where the all-gather degenerates to a copy: both bootstraps (id handed over directly /
    through a file, which rank 0 must remove again once the communicator is up)."""
    from unimatch_amd.dist import RcclGather, make_gather
    dev = torch.device('cuda', torch.cuda.current_device())
    x = rnd(800, 3, 2, 40, 56).to(DEV)
    g = RcclGather(0, 1, dev)
    assert g.ranks() == 1
    out = g.all_gather(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out2 = g.all_gather(x, stream=side)                                       # the side stream bench.py gathers on
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 2, 40, 56) and torch.equal(out[0], x) and torch.equal(out2[0], x)
    g.close()
    path = tmp_path / 'um_rccl_id'
    path.write_bytes(b'stale record of an earlier job' * 8)                   # must be replaced, not trusted
    g = RcclGather(0, 1, dev, id_file=str(path))
    out = g.all_gather(x)
    torch.cuda.synchronize()
    assert torch.equal(out[0], x) and not path.exists()
    g.close()
    gather, kind = make_gather(0, 1, dev)                                      # what bench.py / all_gather_predictions use
    assert 'um_allgather_preds' in kind and gather.ranks() == 1
    gather.close()


def test_survey_named_entry_points(ops):
    """SURVEY.md 8(b)'s literal names (um_swin_attn_fwd, um_attn1d_fwd, um_local_corr_softmax_1d, um_workspace_bytes_<op>) are
    exported and do what the entry points they forward to do: bitwise the same outputs."""
    from unimatch_amd import _abi
    lib = _abi.load()
    st = torch.cuda.current_stream().cuda_stream
    s_, h, w = 2, 16, 24
    q, k, v = (rnd(990 + i, s_, h * w, C).to(DEV) for i in range(3))
    for name, geom, call in (
            ('swin', (8, 12, 4, 6), lambda o, ws: lib.um_swin_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), s_, h, w, C,
                                                                        8, 12, 4, 6, 0, ws.data_ptr(), ws.numel(), st)),
            ('attn1d', (1, 12, 0, 6), lambda o, ws: lib.um_attn1d_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), s_, h, w, C,
                                                                       12, 6, 0, ws.data_ptr(), ws.numel(), st))):
        nbytes = getattr(lib, f'um_workspace_bytes_{"swin_attn_fwd" if name == "swin" else "attn1d_fwd"}')(s_, h, w, C, 0)
        assert nbytes == lib.um_window_attn_workspace_bytes(s_, h * w, C, 0) > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = torch.empty_like(q)
        assert call(out, ws) == 0
        assert torch.equal(out, ops.window_attention(q, k, v, h, w, *geom)), name
    f0, f1 = rnd(995, 2, C, 12, 20), rnd(996, 2, C, 12, 20)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    out = torch.empty(2, 1, 12, 20, device=DEV)
    assert lib.um_local_corr_softmax_1d(t0.data_ptr(), t1.data_ptr(), out.data_ptr(), 2, 12, 20, C, 4, st) == 0
    assert torch.equal(out, ops.local_corr_softmax(t0, t1, 12, 20, 4, one_d=True))
    assert lib.um_workspace_bytes_global_corr_softmax_flow(2, 12, 20, C, 0) == lib.um_global_corr_workspace_bytes(2, 240, C, 0)
    assert lib.um_workspace_bytes_local_corr_with_flow(2, 12, 20, C, 0) == 0 and lib.um_workspace_bytes_allgather_preds(2, 12, 20, C, 0) == 0


def test_per_scale_glue_kernels(ops):
    """um_flow_upsample2x (unimatch.py:162-163), um_depth_cam_pack (K / stride, K^-1, pose and inverse pose in closed form instead of
    torch.inverse) and um_rigid_flow (geometry.py:99-195) against fp64 evaluations of the reference expressions."""
    flow = rnd(1100, 3, 2, 17, 23, scale=4.0)
    want = 2 * torch.nn.functional.interpolate(flow.double(), scale_factor=2, mode='bilinear', align_corners=True)
    got = ops.flow_upsample2x(flow.to(DEV), 2.0)
    assert got.shape == want.shape and err(got, want)[0] < 2e-6 * max(1.0, want.abs().max().item())
    b, h, w = 3, 30, 40
    k, pose = synth_camera(b, 8 * h, 8 * w)
    pose = pose.clone()
    pose[1, :3, 3] *= -2.0                                                     # different poses per sample
    pose[2, :3, :3] = pose[2, :3, :3] @ pose[0, :3, :3]
    kd = k.double().clone()
    kd[:, :2] /= 8.0
    for bidir in (False, True):
        cam = ops.depth_cam(k.to(DEV), pose.to(DEV), 8.0, bidir).cpu().double()
        pd = torch.cat([pose.double(), torch.inverse(pose.double())], 0) if bidir else pose.double()
        kk = kd.repeat(2, 1, 1) if bidir else kd
        want = torch.cat([torch.inverse(kk).flatten(1), pd[:, :3, :3].flatten(1), pd[:, :3, 3], kk.flatten(1)], 1)
        assert cam.shape == want.shape and (cam - want).abs().max().item() < 2e-6 * want.abs().max().item()
    # a singular intrinsics matrix cannot raise from the kernel (torch.inverse would, after a device synchronisation): that sample's
    # K^-1 is all NaN -- nothing half-finite -- and the other samples are untouched (include/unimatch_hip.h, um_depth_cam_pack)
    ks = k.clone()
    ks[1, 1] = ks[1, 0] * 2.0
    cam_s = ops.depth_cam(ks.to(DEV), pose.to(DEV), 8.0, False).cpu()
    good = ops.depth_cam(k.to(DEV), pose.to(DEV), 8.0, False).cpu()
    assert torch.isnan(cam_s[1, :9]).all() and torch.equal(cam_s[0], good[0]) and torch.equal(cam_s[2], good[2])
    inv_depth = (0.2 + rnd(1101, b, 1, h, w).abs()).clamp(0.1, 2.0)
    cam = ops.depth_cam(k.to(DEV), pose.to(DEV), 8.0, False)
    want = om.rigid_flow(1.0 / inv_depth.double().squeeze(1), kd, pose.double())
    got = ops.rigid_flow(inv_depth.to(DEV), cam)
    assert err(got, want)[0] < 5e-5 * max(1.0, want.abs().max().item())


def test_hip_graph_replay_of_the_depth_path():
    """With the camera packing on the device (no torch.inverse) the depth forward has no host synchronisation left: it is captured
    into a HIP graph and replays bitwise equal to eager, also with the refinement step (gmdepth_s1_rr1)."""
    from unimatch_amd.graph import GraphedUniMatch
    for name in ('gmdepth_s1', 'gmdepth_s1_rr1'):
        ck, fk = CONFIGS[name]
        model = UniMatch(**ck).eval()
        model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
        model = model.to(DEV)
        graphed = GraphedUniMatch(model)
        for seed in (25, 26):
            i0, i1 = synth_images(1, 96, 128, seed=seed, kind='shift', normalized=True)
            k, pose = synth_camera(1, 96, 128)
            kw = dict(fk, intrinsics=k.to(DEV), pose=pose.to(DEV))
            want = model(i0.to(DEV), i1.to(DEV), **kw)['flow_preds'][0]
            got = graphed(i0.to(DEV), i1.to(DEV), **kw)['flow_preds'][0]
            assert torch.equal(got, want), (name, seed)
        assert all(v is not False for v in graphed._graphs.values()), name


@pytest.mark.parametrize('dilation', [1, 2, 3])
def test_cost_volume_dilation(ops, dilation):
    """The reference's `dilation` argument of local_correlation_with_flow (matching.py:86-91; 1 in all of its callers): um_local_corr_with_flow_dilated
    against the reference's own gather form in fp64, incl. taps that leave the image."""
    b, h, w = 2, 20, 28
    f0, f1 = rnd(1200, b, C, h, w), rnd(1201, b, C, h, w)
    flow = rnd(1202, b, 2, h, w, scale=3.0)
    want = hp.local_corr_with_flow_dilated(f0.double(), f1.double(), flow.double(), 4, dilation)
    got = ops.local_corr_with_flow(tok(f0).to(DEV), tok(f1).to(DEV), flow.to(DEV), h, w, 4, dilation=dilation)
    assert got.shape == want.shape and err(got, want)[1] < 3e-6 * max(1.0, want.abs().max().item())


def test_operand_range_overflow_is_loud():
    """exact mode has fp16's exponent range.  An activation >= 65504 on its way into an fp16 hi | lo operand
    raises a bit of the library's sticky flag word (um_range_flags) that names the operand; UniMatch.forward / check_operand_range
    turn it into an exception instead of NaN predictions.  Legal magnitudes leave the word at zero; bf16 (fast mode) has no such
    cliff and never raises it."""
    from unimatch_amd import _abi
    ops, fast = HipOps('exact'), HipOps('fast')
    _abi.range_flags(reset=True)
    c, m = 128, 4 * 16 * 24
    x = rnd(970, m, c, scale=1.5).to(DEV)
    y = rnd(971, m, c, scale=1.5).to(DEV)
    w1 = (rnd(972, 8 * c, 2 * c, scale=0.06)).to(DEV)
    w2 = (rnd(973, c, 8 * c, scale=0.03)).to(DEV)
    wq, wk, wv, wm = (rnd(974 + i, c, c, scale=0.09).to(DEV) for i in range(4))
    norm = torch.nn.LayerNorm(c).to(DEV)
    kv, _, n2 = ops.linear_planes(x, (wk, wv))
    attn = lambda o, t: o.window_attention_qproj_merge(t, wq, (kv, m, n2, 0), (kv, m, n2, c), 4, 16, 24, 8, 12, 0, 0, 0, wm, norm, t)
    attn(ops, x)
    ops.ffn_ln(x, y, w1, w2, norm)
    torch.cuda.synchronize()
    assert _abi.range_flags() == 0                                     # the model's magnitudes: nothing raised
    big = x.clone()
    big[5, 7] = 1.0e5                                                   # one activation beyond fp16
    out = attn(ops, big)
    torch.cuda.synchronize()
    flags = _abi.range_flags()
    assert flags & 2 and not torch.isfinite(out).all(), flags          # UM_RANGE_ATTN_TOKENS, and the result really is not finite
    with pytest.raises(_abi.OperandRangeError, match='attention source tokens'):
        _abi.check_operand_range()
    assert _abi.range_flags() == 0                                     # reading through check_* clears the word
    ops.ffn_ln(big, y, w1, w2, norm)
    ops.linear_planes(big, (wk, wv))
    torch.cuda.synchronize()
    flags = _abi.range_flags(reset=True)
    assert flags & 16 and flags & 128, flags                           # UM_RANGE_FFN_TOKENS, UM_RANGE_LINEAR
    ops.ffn_ln(x * 3000.0, y * 3000.0, w1 * 8.0, w2, norm)              # inputs legal (|x| < 3e4), the hidden activations are not
    torch.cuda.synchronize()
    flags = _abi.range_flags(reset=True)
    assert flags & 32 and not flags & 16, flags                        # UM_RANGE_FFN_HIDDEN only
    kvf, _, _ = fast.linear_planes(big, (wk, wv))                       # bf16 operands carry fp32's range: no flag, finite results
    outf = fast.window_attention_qproj_merge(big, wq, (kvf, m, n2, 0), (kvf, m, n2, c), 4, 16, 24, 8, 12, 0, 0, 0, wm, norm, big)
    torch.cuda.synchronize()
    assert _abi.range_flags() == 0 and torch.isfinite(outf).all()
    # the drop-in module: the NEXT forward after an overflow refuses loudly (no synchronisation on the hot path), and
    # check_operand_range() covers the call that has just been made
    model, i0, i1, fk = _graph_case('gmflow_s1', 64, 96)
    model(i0, i1, **fk)
    model.check_operand_range()                                        # clean
    attn(ops, big)
    torch.cuda.synchronize()
    with pytest.raises(_abi.OperandRangeError, match='earlier forward'):
        model(i0, i1, **fk)
    model(i0, i1, **fk)                                                # the flags were cleared by the report
    model.check_operand_range()
