"""GPU tests of the matching confidence: ``um_global_match_stats`` / ``um_match_mutual`` (csrc/match_stats.hip) against
``confidence.global_match_stats_host`` evaluated in float64 on the host.

Shapes (the smallest at which each mechanism can break; the kernel has no key split, so no shape switches kernels):
  5x7 B=1     35 keys: less than one 64-key tile, one (partly empty) query tile
  8x16 B=2    128 keys: exactly two whole tiles
  9x15 B=2    135 keys: a ragged last tile (7 keys) and two query tiles (128 + 7)
  24x40 B=2   960 keys: 15 tiles, 8 query tiles
  stereo 6x40, 3x70   the causal diagonal inside one tile, and across two tiles

Inputs: ``f0 = a u`` with a per-query gain ``a`` log-uniform in [0.02, 1.5] and ``f1`` a permuted (stereo: shifted) copy of ``u`` plus
noise, so that the float64 ``max_prob`` runs from below 0.05 to above 0.9 within a case (asserted; for stereo the upper end is taken
over the columns x > 0, because the one-key rows at x = 0 are 1 whatever the features are).  The adversary flips the sign of half the
keys at gain 5.3: logits reach +-60 and the running offset is rescaled again and again.  Planted rows: chosen queries are replaced by
a multiple of a chosen key, which makes that key the row's best by a float64 logit gap >= 1 (asserted); ``best`` must hit it exactly.

Gate of a float output (max abs distance to float64):  kernel <= 2 x (float32 host restatement on the same inputs) + floor.  2 x is
the project's stage-parity gate.  The floor is what the kernel's ARITHMETIC ORDER costs next to the restatement's, and it is worked
out, not read off a run (a floor read off the kernel's own error would pass whatever the kernel does): the restatement sums every row
pairwise (torch.sum) and centres the coordinates before squaring them, the kernel runs ONE sequential fp32 chain per lane over n = L / 2
keys and takes the variance as E|d|^2 - |E d|^2.  With u = 2^-24 (half an fp32 ulp) the error of a chain of n rounded additions is a
random walk of standard deviation sqrt(n) u times the accumulated magnitude.  The constant 8 is 4 x 2: the largest of the 10^3 .. 10^4
rows of a case sits about 4 standard deviations out, and every statistic is a quotient of TWO such chains (its numerator and l; the
variance subtracts two quotients of the same size).  So floor = 8 sqrt(L / 2) 2^-24 x scale, scale = the largest magnitude the
numerator chain can reach per unit of l: 1 (max_prob), ln L (entropy: its largest value), max(h, w) (mean: the largest displacement),
h^2 + w^2 (variance: the largest second moment about the query's own pixel; stereo: w and w^2).  The deterministic worst case of the
same chain, n u x scale, is sqrt(n) / 8 times larger (2.7 x at L = 960): the floor is well inside it.  profiles/match_stats.txt records
the measured distances next to the floor (the kernel's largest share of it there is 0.4: max_prob at 24x40).
Fast mode compares against the float64 evaluation of the operands as the kernel rounds them: ``bf16(f x plane scale)``."""
import math

import pytest
import torch

from unimatch_amd import _abi, confidence
from unimatch_amd.ops import HipOps
from tests import memory_guard as mg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 128
FLOW_SHAPES = [(1, 5, 7), (2, 8, 16), (2, 9, 15), (2, 24, 40)]
STEREO_SHAPES = [(2, 6, 40), (2, 3, 70)]
CASES = [('flow',) + s for s in FLOW_SHAPES] + [('stereo',) + s for s in STEREO_SHAPES] + [('adversary', 2, 9, 15)]
FIELDS = ('max_prob', 'entropy', 'variance', 'mean')


def make_inputs(kind, b, h, w, seed=0):
    """``(f0, f1, planted)``: float32 host features ``[B, h*w, C]`` and the planted ``(batch, query, key)`` triples."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    l = h * w
    u = torch.randn(b, l, C, generator=g)
    if kind == 'stereo':
        src = u.view(b, h, w, C).roll(-2, dims=2).reshape(b, l, C)         # key x' carries query x' + 2: the match lies 2 to the left
    else:
        perm = torch.stack([torch.randperm(l, generator=g) for _ in range(b)])
        src = u.gather(1, perm[:, :, None].expand(b, l, C))
    f1 = src + 0.3 * torch.randn(b, l, C, generator=g)
    if kind == 'adversary':
        sign = torch.where(torch.rand(b, l, 1, generator=g) < 0.5, -1.0, 1.0)
        f0, f1 = 5.3 * u, sign * f1
    else:
        gain = torch.exp(torch.empty(b, l, 1).uniform_(math.log(0.02), math.log(1.5), generator=g))
        f0 = gain * u
    planted = []
    if kind == 'stereo':
        for row, x, key in ((0, w - 1, w - 1), (h - 1, w - 1, 0), (1, w // 2, w // 2), (h - 1, 3, 3), (0, w - 2, 64 % w)):
            planted.append((0, row * w + x, row * w + min(key, x)))         # on the diagonal, at column 0, in the second tile
    else:
        tail = 64 * ((l - 1) // 64)                                         # first key of the (ragged) last tile
        for q, key in ((1, 0), (l // 2, l - 1), (l - 1, tail), (0, min(tail + 3, l - 1)), (l // 3, l // 2)):
            planted.append((b - 1, q, key))
    for bi, q, key in planted:
        k = f1[bi, key]
        f0[bi, q] = k * (14.0 * math.sqrt(C) / float(k @ k))               # logit 14 at the key; the others stay a few units
    return f0.contiguous(), f1.contiguous(), planted


def logits64(f0, f1, h, w, stereo):
    b, l, c = f0.shape
    if stereo:
        s = f0.view(b, h, w, c) @ f1.view(b, h, w, c).transpose(-1, -2) / c ** 0.5
        right = torch.triu(torch.ones(w, w, dtype=torch.bool), diagonal=1)
        return s.masked_fill(right, float('-inf')).view(b, l, w)
    return f0 @ f1.transpose(-1, -2) / c ** 0.5


def as_rounded(f, precision):
    """The operands the kernel multiplies, as float32 features: fast mode rounds ``f x plane scale`` to bf16 (planes.h)."""
    if precision == 'exact':
        return f
    scale = torch.tensor(_abi.load().um_global_corr_plane_scale(C), dtype=torch.float32)
    return (f * scale).bfloat16().float() / scale.double()


def floors(h, w, stereo):
    l = w if stereo else h * w
    c = 8.0 * math.sqrt(l / 2.0) * 2.0 ** -24
    span = w if stereo else max(h, w)
    return {'max_prob': c, 'entropy': c * math.log(l), 'mean': c * span, 'variance': c * (w * w if stereo else h * h + w * w)}


_reference_cache = {}


def reference(kind, b, h, w, precision):
    """Inputs, the float64 reference on the operands of ``precision`` and the float32 restatement: computed once per case."""
    key = (kind, b, h, w, precision)
    if key not in _reference_cache:
        stereo = kind == 'stereo'
        f0, f1, planted = make_inputs(kind, b, h, w)
        r0, r1 = as_rounded(f0, precision), as_rounded(f1, precision)
        ref64 = confidence.global_match_stats_host(r0.double(), r1.double(), h, w, stereo=stereo)
        ref32 = confidence.global_match_stats_host(r0.float(), r1.float(), h, w, stereo=stereo)
        lg64 = logits64(r0.double(), r1.double(), h, w, stereo)
        lg32 = logits64(r0.float(), r1.float(), h, w, stereo)
        finite = torch.isfinite(lg64)
        lg_err = (lg32.double() - lg64)[finite].abs().max().item()
        _reference_cache[key] = (f0, f1, planted, ref64, ref32, lg64, lg_err)
    return _reference_cache[key]


def gate(name, got, r64, r32, floor, what):
    d = (got.detach().double().cpu() - r64).abs().max().item()
    d32 = (r32.double() - r64).abs().max().item()
    print(f'{what} {name}: kernel {d:.3e}  float32 host {d32:.3e}  floor {floor:.3e}  bound {2 * d32 + floor:.3e}')
    assert math.isfinite(d) and d <= 2 * d32 + floor, (what, name, d, d32, floor)


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('kind,b,h,w', CASES, ids=[f'{k}-{b}x{h}x{w}' for k, b, h, w in CASES])
def test_stats_against_float64(kind, b, h, w, precision):
    stereo = kind == 'stereo'
    f0, f1, planted, ref64, ref32, lg64, lg_err = reference(kind, b, h, w, precision)
    if kind == 'flow':
        assert ref64.max_prob.min() < 0.05 and ref64.max_prob.max() > 0.9, (ref64.max_prob.min(), ref64.max_prob.max())
    elif stereo:
        assert ref64.max_prob.min() < 0.05 and ref64.max_prob[..., 1:].max() > 0.9, (ref64.max_prob.min(), ref64.max_prob[..., 1:].max())
    else:
        assert lg64.max() > 55 and lg64.min() < -55
    got = confidence.global_match_stats(f0.to(DEV), f1.to(DEV), h, w, stereo=stereo, precision=precision)
    what = f'{kind} {b}x{h}x{w} {precision}'
    fl = floors(h, w, stereo)
    for name in FIELDS:
        gate(name, getattr(got, name), getattr(ref64, name), getattr(ref32, name), fl[name], what)
    assert bool((got.entropy >= 0).all()) and bool((got.variance >= 0).all()) and bool((got.max_prob <= 1).all())
    # best: exact on the planted rows (none excluded), elsewhere a key whose float64 logit is the row maximum to within the tolerance
    best = got.best.cpu().view(b, -1).long()
    nkeys = lg64.shape[-1]
    assert bool(((best >= 0) & (best < nkeys)).all())
    top2 = lg64.topk(2, -1).values
    for bi, q, key in planted:
        assert top2[bi, q, 0] - top2[bi, q, 1] >= 1.0, (what, 'planted gap', bi, q)
        want = key % w if stereo else key
        assert int(lg64[bi, q].argmax()) == want
        assert int(best[bi, q]) == want, (what, 'planted row', bi, q, int(best[bi, q]), want)
    at_best = lg64.gather(-1, best[..., None])[..., 0]
    tol = 2 * lg_err + lg64[torch.isfinite(lg64)].abs().max().item() * 2.0 ** -20
    assert bool((at_best >= top2[..., 0] - tol).all()), (what, (top2[..., 0] - at_best).max().item(), tol)
    if stereo:                                                              # one key at x = 0: exactly certain
        first = slice(None), slice(None), 0
        assert bool((got.max_prob[first] == 1).all()) and bool((got.entropy[first] == 0).all()) and bool((got.variance[first] == 0).all())
        assert bool((got.best[first] == 0).all()) and bool((got.mean[:, 0][first] == 0).all())


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('kind,b,h,w', [('flow', 2, 9, 15), ('flow', 2, 24, 40), ('stereo', 2, 6, 40), ('stereo', 2, 3, 70)])
def test_mean_against_the_matching_entry_points(kind, b, h, w, precision):
    """``mean`` next to ``um_global_corr_softmax_flow`` / ``_stereo`` on the same inputs: both within the gate of the float64 value
    (the same tolerance rule; bitwise equality is not required)."""
    stereo = kind == 'stereo'
    f0, f1, _, ref64, ref32, _, _ = reference(kind, b, h, w, precision)
    ops = HipOps(precision)
    d0, d1 = f0.to(DEV), f1.to(DEV)
    got = confidence.global_match_stats(d0, d1, h, w, stereo=stereo, precision=precision).mean
    entry = -ops.global_corr_softmax_stereo(d0, d1, h, w) if stereo else ops.global_corr_softmax_flow(d0, d1, h, w)
    fl = floors(h, w, stereo)['mean']
    what = f'{kind} {b}x{h}x{w} {precision}'
    gate('mean', got, ref64.mean, ref32.mean, fl, what)
    gate('entry point', entry, ref64.mean, ref32.mean, fl, what)
    d32 = (ref32.mean.double() - ref64.mean).abs().max().item()
    assert (got - entry).abs().max().item() <= 2 * (2 * d32 + fl)


@pytest.mark.parametrize('precision', ['exact', 'fast'])
def test_bidir_is_the_swapped_launch_bitwise(precision):
    b, h, w = 2, 9, 15
    f0, f1, _ = make_inputs('flow', b, h, w, seed=5)
    d0, d1 = f0.to(DEV), f1.to(DEV)
    both = confidence.global_match_stats(d0, d1, h, w, bidir=True, precision=precision)
    fwd = confidence.global_match_stats(d0, d1, h, w, precision=precision)
    bwd = confidence.global_match_stats(d1, d0, h, w, precision=precision)
    for name in FIELDS + ('best',):
        assert tuple(getattr(both, name).shape[:1]) == (2 * b,)
        assert torch.equal(getattr(both, name)[:b], getattr(fwd, name)), name
        assert torch.equal(getattr(both, name)[b:], getattr(bwd, name)), name


def test_mean_is_optional_in_the_abi():
    """``mean = NULL``: the other outputs are the same bytes, and the call reports nothing."""
    b, h, w = 2, 9, 15
    f0, f1, _ = make_inputs('flow', b, h, w, seed=6)
    d0, d1 = f0.to(DEV), f1.to(DEV)
    lib = _abi.load()
    want = confidence.global_match_stats(d0, d1, h, w)
    stats = torch.empty((b, 3, h, w), dtype=torch.float32, device=DEV)
    best = torch.empty((b, h, w), dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.um_global_match_stats_workspace_bytes(b, h * w, C, 0), dtype=torch.uint8, device=DEV)
    _abi.check(lib.um_global_match_stats(d0.data_ptr(), d1.data_ptr(), stats.data_ptr(), best.data_ptr(), None, b, h, w, C, 0, 0, 0,
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), 'um_global_match_stats')
    assert torch.equal(stats[:, 0], want.max_prob) and torch.equal(stats[:, 1], want.entropy) and torch.equal(stats[:, 2], want.variance)
    assert torch.equal(best, want.best)


@pytest.mark.parametrize('radius', [0, 1, 2])
def test_mutual_against_the_host(radius):
    b, h, w = 2, 9, 15
    l = h * w
    g = torch.Generator().manual_seed(77)
    fwd = torch.stack([torch.randperm(l, generator=g) for _ in range(b)]).int()
    bwd = torch.argsort(fwd.long(), 1).int()                               # the inverse permutation: every query mutual
    move = torch.rand(b, l, generator=g) < 0.4                             # ... then 40 % of the keys look a few pixels elsewhere
    bwd = torch.where(move, (bwd + torch.randint(-w - 2, w + 3, (b, l), generator=g).int()).clamp(0, l - 1), bwd)
    bwd[0, 5], fwd[1, 7], fwd[1, 9] = -1, l, -3                            # invalid indices are no match, and nothing is read through them
    fwd, bwd = fwd.view(b, h, w), bwd.view(b, h, w)
    want = confidence.mutual_matches_host(fwd, bwd, h, w, radius)
    got = confidence.mutual_matches(fwd.to(DEV), bwd.to(DEV), h, w, radius)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want)
    assert 0 < int(want.sum()) < b * l


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('kind,b,h,w', [('flow', 2, 9, 15), ('stereo', 2, 3, 70)])
def test_memory_contract(kind, b, h, w, precision):
    """Red zones intact, inputs unchanged, results identical across the fills: every element of stats, best and mean is written and
    nothing is read beyond the inputs and the workspace.  The mutual check rides on the flow case."""
    stereo = kind == 'stereo'

    def run(_, g):
        f0, f1, _ = make_inputs(kind, b, h, w, seed=9)
        s = confidence.global_match_stats(g.place(f0), g.place(f1), h, w, bidir=not stereo, stereo=stereo, precision=precision)
        out = [s.max_prob, s.entropy, s.variance, s.best, s.mean]
        if not stereo:
            out.append(confidence.mutual_matches(g.place(s.best[:b].cpu()), g.place(s.best[b:].cpu()), h, w, 1))
        return out

    first = mg.contract(run, lambda guard: (guard,), device=DEV)
    assert first is not None
    assert any('confidence.py' in site for site in mg.contract.last_sites)


# ------------------------------------------------------------------ the model method
def _model(name, precision='exact'):
    from unimatch_amd import UniMatch
    from unimatch_amd.synth import CONFIGS, synth_state_dict
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    return model.to(DEV).set_precision(precision), dict(fk)


@pytest.mark.parametrize('name,size,precision', [('gmflow_s1', (64, 96), 'exact'), ('gmflow_s1', (96, 128), 'exact'), ('gmflow_s1', (64, 96), 'fast'),
                                                 ('gmstereo_s1', (64, 96), 'exact'), ('gmstereo_s1', (96, 128), 'exact'),
                                                 ('gmstereo_s1', (96, 128), 'fast')])
def test_forward_with_confidence(name, size, precision):
    from unimatch_amd.synth import synth_frames
    model, kw = _model(name, precision)
    bidir = kw['task'] == 'flow'
    if bidir:
        kw['pred_bidir_flow'] = True
    frames = synth_frames(3, size[0], size[1], seed=2200).to(DEV)
    img0, img1 = frames[:2].contiguous(), frames[1:].contiguous()
    model.launch_parts = 1
    plain = model(img0, img1, **kw)
    out = model.forward_with_confidence(img0, img1, **kw)
    assert all(torch.equal(a, b) for a, b in zip(out['flow_preds'], plain['flow_preds']))
    assert 'match_confidence' not in plain
    model.debug_taps = taps = {}                                           # the taps of the very forward the confidence comes from
    conf = model.forward_with_confidence(img0, img1, **kw)['match_confidence']
    model.debug_taps = None
    h, w = size[0] // 8, size[1] // 8
    t0, t1 = (taps[k].flatten(2).transpose(1, 2).contiguous() for k in ('f0_s0', 'f1_s0'))
    want = confidence.global_match_stats(t0, t1, h, w, bidir=bidir, stereo=not bidir, precision=precision)   # the model's own operand format
    assert conf['scale'] == 8 and tuple(conf['max_prob'].shape) == (4 if bidir else 2, h, w)
    for key in ('max_prob', 'entropy', 'variance', 'best'):
        assert torch.equal(conf[key], getattr(want, key)), key
    if precision == 'fast':                                                # ... and not the other one
        other = confidence.global_match_stats(t0, t1, h, w, bidir=bidir, stereo=not bidir, precision='exact')
        assert not torch.equal(conf['entropy'], other.entropy)
    if bidir:
        assert torch.equal(conf['mutual'], confidence.mutual_matches(want.best[:2], want.best[2:], h, w, 0))
    else:
        assert 'mutual' not in conf


def test_forward_sequence_confidence_is_taken_in_its_own_forward():
    """``forward_sequence(return_confidence=True)``: the flows are those of the plain call bit for bit, and the maps are those of the
    pairwise ``forward_with_confidence`` (the encoder batch differs: the maps agree to 1e-4 of their range, the arg-max away from
    near-ties, as tests/test_match_stats_cpu.py has it for the host path)."""
    from unimatch_amd.synth import synth_frames
    model, kw = _model('gmflow_s1')
    kw.pop('task')
    frames = synth_frames(4, 64, 96, seed=2203).to(DEV)
    want = model.forward_with_confidence(frames[:-1].contiguous(), frames[1:].contiguous(), pred_bidir_flow=True, **kw)['match_confidence']
    plain = model.forward_sequence(frames, pred_bidir_flow=True, pairs_per_launch=2, **kw)
    out = model.forward_sequence(frames, pred_bidir_flow=True, pairs_per_launch=2, return_confidence=True, **kw)
    assert torch.equal(out['flow'], plain['flow']) and torch.equal(out['flow_bwd'], plain['flow_bwd']) and 'match_confidence' not in plain
    conf = out['match_confidence']
    for key in ('max_prob', 'entropy', 'variance'):
        assert tuple(conf[key].shape) == (3, 8, 12)
        assert (conf[key] - want[key][:3]).abs().max().item() <= 1e-4 * max(1.0, want[key].abs().max().item()), key
    assert (conf['best'] == want['best'][:3]).float().mean() >= 0.98 and (conf['mutual'] == want['mutual']).float().mean() >= 0.98


def test_forward_with_confidence_refuses_depth():
    from unimatch_amd.synth import synth_frames
    model, kw = _model('gmdepth_s1')
    frames = synth_frames(2, 64, 96, seed=2201).to(DEV)
    with pytest.raises(NotImplementedError, match='plane sweep'):
        model.forward_with_confidence(frames[:1], frames[1:], intrinsics=torch.eye(3, device=DEV)[None], pose=torch.eye(4, device=DEV)[None], **kw)
