"""``um_depth_corr_softmax_stats`` on the device: the plane sweep's prediction and the statistics of its distribution in one launch,
against the float64 host restatement (``confidence.depth_match_logits_host`` on the same float32 values), through both K7 kernels
(box: D <= 64 with the per-pixel gather fallback; gather: D > 64), the exact cases (nothing in view, one candidate), the
self-consistency of the one launch, the plain kernel, the optional outputs, the memory contract and the model methods.

Gates.  Float planes: max abs distance to float64 at most ``2e-4 * scale`` -- the tolerance tests/test_hip_parity_gpu.py applies to
this kernel's soft-argmin output; the logits and exponentials are the same -- with ``scale`` 1 for ``max_prob`` and ``peak_mass``,
``max(1, ln D)`` for ``entropy``, ``max(cand)`` for ``out`` and ``(max(cand) - min(cand))^2`` for ``variance``.  ``best``: in range; the
float64 probability of the kernel's pick within 2e-4 of the row maximum (no row excluded); equal to the float64 arg-max wherever the
top two float64 logits are at least 0.1 apart.  ``in_view``: equal to the float64 count wherever no candidate of the pixel lands
within 1e-3 of a coordinate at which the count changes (x = -1 or w, y = -1 or h; fewer pixels are excluded than by "any integer").
The inputs' own properties (distributions from flat to peaked, candidates leaving the view, boxes on both sides of the table size)
are asserted on the float64 reference, so the inputs cannot go soft.  Measured distances: profiles/depth_match_stats.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import memory_guard as mg
from unimatch_amd import _abi, confidence
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 128
TOL = 2e-4
DEPTH_BOX = 160               # csrc/local_ops.hip: a pixel whose candidates' corners span more table rows takes the per-pixel gather
SHAPES = [(1, 1, 1), (2, 9, 11), (2, 16, 24)]      # one pixel | 198 pixels: no multiple of a workgroup's 4 waves | the fallback's size
COUNTS = [1, 5, 17, 64, 65, 128]                   # degenerate | idle lanes | one past a 16-slot round | full wave | gather kernel: first, last
MOVES = {'sideways': (0.12, -0.01, 0.0), 'diagonal': (0.45, 0.40, 0.0), 'forward': (0.02, 0.01, 0.30), 'away': (15.0, 0.0, 0.0)}
FLOATS = ('max_prob', 'entropy', 'variance', 'peak_mass')
# Cases in which more than 5 % of the pixels have a candidate within 1e-3 of a coordinate at which in_view changes, by geometry: 65 or
# 128 candidates 0.1 - 0.2 cells apart crossing one to three such coordinates per pixel (2e-3 / spacing each).  They keep 91 - 94 %.
DENSE_CROSSINGS = {(9, 11, 65, 'sideways'), (9, 11, 65, 'diagonal'), (16, 24, 128, 'diagonal')}


# ------------------------------------------------------------------ inputs and the float64 reference
@functools.lru_cache(maxsize=None)
def features(b, h, w):
    """Token-major ``f0``, ``f1`` ``[B, h*w, 128]`` float32: the second view is the first shifted by two columns plus noise, and the
    first carries a per-pixel gain log-uniform in [0.05, 3], so that the distributions run from flat to peaked (logits to about 20)."""
    g = torch.Generator().manual_seed(9001 + 100 * h + w)
    f0 = torch.randn(b, C, h, w, generator=g)
    f1 = 0.6 * f0.roll(2, dims=-1) + 0.4 * torch.randn(b, C, h, w, generator=g)
    gain = torch.exp(torch.rand(b, 1, h, w, generator=g) * math.log(3 / 0.05) + math.log(0.05))
    return tuple((f.flatten(2).transpose(1, 2).contiguous()) for f in (f0 * gain, f1))


def camera(b, h, w, move):
    """The packed ``cam [B, 30]`` float32 of tests/test_hip_parity_gpu.py's plane-sweep cases: fx = 0.9 w, centre (w/2, h/2)."""
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    pose[:, :3, 3] = torch.tensor(MOVES[move])
    if move == 'forward' and b > 1:
        a = 0.04
        pose[1, :3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    return torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous()


def candidates(d):
    return torch.linspace(1 / 10.0, 1 / 0.5, d)


@functools.lru_cache(maxsize=None)
def reference(b, h, w, d, move):
    """float64, computed once per case and shared: logits, prob, the statistics at ``peak_radius`` 1, the soft-argmin, and per pixel
    whether ``in_view`` is decided clear of the fp32 rounding of the coordinates."""
    f0, f1 = features(b, h, w)
    cam, cand = camera(b, h, w, move).double(), candidates(d).double()
    logits, seen = confidence.depth_match_logits_host(f0.double(), f1.double(), h, w, cam, cand)
    prob = torch.softmax(logits, 1)
    stats = confidence.depth_stats_from_prob_host(prob, cand, seen, 1)
    clear, gap, sx, sy = clear_and_gap(h, w, cam, cand, logits)
    return dict(logits=logits, prob=prob, stats=stats, out=(prob * cand.view(1, d, 1, 1)).sum(1, keepdim=True), clear=clear,
                gap=gap, sx=sx, sy=sy)


def clear_and_gap(h, w, cam, cand, logits):
    """Per pixel, from float64: ``clear`` -- no candidate lands within 1e-3 of a coordinate at which ``in_view`` changes (x = -1 or w,
    y = -1 or h) -- and ``gap``, the distance of the top two logits; with the coordinates."""
    d = cand.numel()
    sx, sy = confidence.depth_sample_coords_host(h, w, cam, cand)
    near = torch.zeros_like(sx, dtype=torch.bool)
    for coord, hi in ((sx, w), (sy, h)):
        for edge in (-1.0, float(hi)):
            near |= (coord - edge).abs() < 1e-3
    top = logits.topk(min(2, d), 1)[0]
    gap = (top[:, 0] - top[:, 1]) if d > 1 else torch.full_like(top[:, 0], float('inf'))
    return ~near.any(1), gap, sx, sy


def box_positions(b, h, w, d, move):
    """Per pixel, the size of the bounding box of the candidates' corners as the box kernel computes it (from the float64 coordinates)."""
    ref = reference(b, h, w, d, move)
    x0 = torch.floor(ref['sx']).clamp(-1, w - 1)
    y0 = torch.floor(ref['sy']).clamp(-1, h - 1)
    return (x0.amax(1) + 1 - x0.amin(1) + 1) * (y0.amax(1) + 1 - y0.amin(1) + 1)


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


def launch(ops, b, h, w, d, move, from_argmax=False, peak_radius=1):
    f0, f1 = features(b, h, w)
    return ops.depth_corr_softmax(f0.to(DEV), f1.to(DEV), h, w, camera(b, h, w, move).to(DEV), candidates(d).to(DEV), from_argmax,
                                  stats=True, peak_radius=peak_radius)


def scales(d):
    cand = candidates(d)
    return {'max_prob': 1.0, 'peak_mass': 1.0, 'entropy': max(1.0, math.log(d)), 'out': cand.max().item(),
            'variance': (cand.max() - cand.min()).item() ** 2}


# ------------------------------------------------------------------ the inputs' own properties, on the float64 reference
def test_the_inputs_span_what_the_gates_need():
    for h, w in ((9, 11), (16, 24)):
        mp = reference(2, h, w, 5, 'sideways')['stats'].max_prob
        assert mp.min() <= 0.21 and mp.max() >= 0.99, (h, w, mp.min(), mp.max())
    s = reference(2, 16, 24, 64, 'sideways')['stats']
    assert s.max_prob.min() <= 1.05 / 64 and s.max_prob.max() > 0.5, (s.max_prob.min(), s.max_prob.max())     # flat rows: a gain of 0.05
    assert s.entropy.min() < 1.5 and s.entropy.max() >= math.log(64) - 1e-3, (s.entropy.min(), s.entropy.max())
    assert reference(2, 16, 24, 64, 'diagonal')['stats'].in_view.max() < 64
    partly = (reference(2, 9, 11, 64, 'sideways')['stats'].in_view < 64).float().mean().item()
    assert 0.1 <= partly <= 0.4, partly
    for b, h, w in SHAPES:
        assert bool((reference(b, h, w, 64, 'away')['stats'].in_view == 0).all())
    npos = box_positions(2, 16, 24, 64, 'diagonal')
    assert (npos > DEPTH_BOX + 20).any() and (npos < DEPTH_BOX - 20).any(), (npos.min(), npos.max())
    assert (box_positions(2, 16, 24, 64, 'sideways') < DEPTH_BOX - 20).all()
    assert reference(2, 16, 24, 64, 'sideways')['logits'].abs().max() > 10
    # near-ties are common: best is gated by value, and by equality only where the float64 gap is wide -- which must stay a real share
    assert (reference(2, 16, 24, 64, 'sideways')['gap'] >= 0.1).float().mean() >= 0.25
    assert (reference(2, 16, 24, 5, 'sideways')['gap'] >= 0.1).float().mean() >= 0.60
    # in_view is compared away from the coordinates at which it changes: that keeps at least 95 % of the pixels over all cases, and in
    # every case but DENSE_CROSSINGS (asserted per case in test_stats_against_float64)
    clear = torch.cat([reference(b, h, w, d, move)['clear'].flatten() for b, h, w in SHAPES for d in COUNTS for move in MOVES])
    assert clear.float().mean().item() >= 0.95, clear.float().mean().item()


# ------------------------------------------------------------------ against float64
@pytest.mark.parametrize('move', list(MOVES))
@pytest.mark.parametrize('d', COUNTS)
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_stats_against_float64(ops, b, h, w, d, move):
    ref = reference(b, h, w, d, move)
    out, stats, index = (t.cpu() for t in launch(ops, b, h, w, d, move))
    assert tuple(out.shape) == (b, 1, h, w) and tuple(stats.shape) == (b, 4, h, w) and tuple(index.shape) == (b, 2, h, w)
    assert index.dtype == torch.int32 and bool(torch.isfinite(stats).all()) and bool(torch.isfinite(out).all())
    sc = scales(d)
    dist = {'out': (out.double() - ref['out']).abs().max().item()}
    for i, name in enumerate(FLOATS):
        dist[name] = (stats[:, i].double() - getattr(ref['stats'], name)).abs().max().item()
    print(f'{b}x{h}x{w} D={d} {move}: ' + ' '.join(f'{k} {v:.2e}/{TOL * sc[k]:.2e}' for k, v in dist.items()))
    for name, v in dist.items():
        assert v <= TOL * sc[name], (name, v, TOL * sc[name])
    best, seen = index[:, 0].long(), index[:, 1]
    assert bool((best >= 0).all()) and bool((best < d).all())
    picked = ref['prob'].gather(1, best[:, None])[:, 0]
    assert (ref['prob'].amax(1) - picked).max().item() <= TOL                      # value optimality: no row excluded
    wide = ref['gap'] >= 0.1
    assert torch.equal(best[wide], ref['prob'].argmax(1)[wide])
    clear = ref['clear']                 # kept: >= 95 % of the pixels, but for the three cases of DENSE_CROSSINGS (>= 90 % there)
    assert clear.float().mean().item() >= (0.90 if (h, w, d, move) in DENSE_CROSSINGS else 0.95)
    assert torch.equal(seen[clear], ref['stats'].in_view[clear])
    assert bool((seen >= 0).all()) and bool((seen <= d).all())
    print(f'    best == float64 arg-max on {(best == ref["prob"].argmax(1)).float().mean().item():.3f} of the rows '
          f'(wide gap: {wide.float().mean().item():.3f}); in_view compared on {clear.float().mean().item():.3f}')


@pytest.mark.parametrize('d', COUNTS)
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_nothing_in_view_is_exactly_uniform(ops, b, h, w, d):
    out, stats, index = (t.cpu() for t in launch(ops, b, h, w, d, 'away'))
    assert bool((index == 0).all())                                                # best == 0 and in_view == 0
    one_over = np.float32(1.0) / np.float32(d)
    assert (stats[:, 0].double() - 1.0 / d).abs().max().item() <= float(np.spacing(one_over))
    ln = np.float32(math.log(d))
    assert (stats[:, 1].double() - math.log(d)).abs().max().item() <= float(np.spacing(ln)) if d > 1 else bool((stats[:, 1] == 0).all())
    assert (out.double() - candidates(d).double().mean()).abs().max().item() <= TOL * scales(d)['out']


@pytest.mark.parametrize('move', ['sideways', 'diagonal', 'forward'])
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_one_candidate_is_exactly_certain(ops, b, h, w, move):
    out, stats, index = (t.cpu() for t in launch(ops, b, h, w, 1, move, peak_radius=0))
    assert bool((stats[:, 0] == 1).all()) and bool((stats[:, 1] == 0).all()) and bool((stats[:, 2] == 0).all()) and bool((stats[:, 3] == 1).all())
    assert bool((index[:, 0] == 0).all()) and bool((out == candidates(1)[0]).all())


# ------------------------------------------------------------------ self-consistency inside the one launch
@pytest.mark.parametrize('move', ['sideways', 'diagonal'])
@pytest.mark.parametrize('d', [17, 64, 80, 128])
@pytest.mark.parametrize('b,h,w', SHAPES[1:])
def test_self_consistency_of_one_launch(ops, b, h, w, d, move):
    cand = candidates(d).to(DEV)
    out, stats, index = launch(ops, b, h, w, d, move, from_argmax=True, peak_radius=0)
    assert torch.equal(out[:, 0], cand[index[:, 0].long()])                        # the read-out is the candidate at best, bit for bit
    assert torch.equal(stats[:, 3], stats[:, 0])                                   # radius 0: peak_mass is max_prob, bit for bit
    soft, wide, index2 = launch(ops, b, h, w, d, move, peak_radius=128)
    assert (wide[:, 3] - 1).abs().max().item() <= TOL
    assert torch.equal(index2, index) and torch.equal(wide[:, :3], stats[:, :3])   # neither flag touches the other outputs
    ref = reference(b, h, w, d, move)
    assert (soft.cpu().double() - ref['out']).abs().max().item() <= TOL * scales(d)['out']


@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('d,move', [(5, 'sideways'), (64, 'sideways'), (64, 'diagonal'), (64, 'forward'), (65, 'sideways'), (128, 'forward')])
@pytest.mark.parametrize('b,h,w', SHAPES[1:])
def test_against_the_plain_kernel(ops, b, h, w, d, move, argmax):
    f0, f1 = (f.to(DEV) for f in features(b, h, w))
    cam, cand = camera(b, h, w, move).to(DEV), candidates(d).to(DEV)
    plain = ops.depth_corr_softmax(f0, f1, h, w, cam, cand, argmax)
    fused = ops.depth_corr_softmax(f0, f1, h, w, cam, cand, argmax, stats=True)[0]
    print(f'{b}x{h}x{w} D={d} {move} argmax={argmax}: fused out bitwise equal to the plain kernel: {torch.equal(plain, fused)}')
    if argmax:                       # both read cand[first arg-max] of the same logits: any difference would be another candidate
        assert torch.equal(plain, fused)
    assert (plain - fused).abs().max().item() <= TOL * scales(d)['out']


@pytest.mark.parametrize('d,move', [(64, 'diagonal'), (80, 'sideways')])
def test_stats_and_index_are_optional_in_the_abi(d, move):
    b, h, w = 2, 16, 24
    lib = _abi.load()
    f0, f1 = (f.to(DEV) for f in features(b, h, w))
    cam, cand = camera(b, h, w, move).to(DEV), candidates(d).to(DEV)

    def call(with_stats, with_index):
        out = torch.full((b, 1, h, w), float('nan'), device=DEV)
        stats = torch.full((b, 4, h, w), -7.0, device=DEV)
        index = torch.full((b, 2, h, w), -7, dtype=torch.int32, device=DEV)
        _abi.check(lib.um_depth_corr_softmax_stats(f0.data_ptr(), f1.data_ptr(), cam.data_ptr(), cand.data_ptr(), out.data_ptr(),
                                                   stats.data_ptr() if with_stats else None, index.data_ptr() if with_index else None,
                                                   b, h, w, C, d, 0, 1, torch.cuda.current_stream().cuda_stream), 'um_depth_corr_softmax_stats')
        return out, stats, index

    out, stats, index = call(True, True)
    o1, s1, i1 = call(False, True)
    o2, s2, i2 = call(True, False)
    o3, s3, i3 = call(False, False)
    assert torch.equal(o1, out) and torch.equal(o2, out) and torch.equal(o3, out)
    assert torch.equal(i1, index) and torch.equal(s2, stats)
    assert bool((s1 == -7).all()) and bool((i2 == -7).all()) and bool((s3 == -7).all()) and bool((i3 == -7).all())     # not written


# ------------------------------------------------------------------ memory contract
@pytest.mark.parametrize('b,h,w', SHAPES[1:])
def test_memory_contract(b, h, w):
    """Red zones intact, inputs unchanged, results identical across the fills: every byte of out, stats and index is written, nothing
    outside them, and nothing is read beyond the inputs.  The box path, the long diagonal (the per-pixel fallback, reached at 16x24),
    the gather kernel (80 candidates) and the arg-max read-out."""
    if h == 16:
        npos = box_positions(b, h, w, 64, 'diagonal')
        assert (npos > DEPTH_BOX + 20).any() and (npos < DEPTH_BOX - 20).any()

    def run(ops, g):
        f0, f1 = (g.place(f) for f in features(b, h, w))
        res = []
        for move, d, argmax in (('sideways', 64, False), ('diagonal', 64, False), ('sideways', 80, False), ('forward', 64, True),
                                ('forward', 80, True)):
            res += list(ops.depth_corr_softmax(f0, f1, h, w, g.place(camera(b, h, w, move)), g.place(candidates(d)), argmax,
                                               stats=True, peak_radius=2))
        return res

    first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps('exact'))
    assert first is not None
    assert any('ops.py' in site for site in mg.contract.last_sites)


# ------------------------------------------------------------------ the model methods
def _model(name):
    from unimatch_amd import UniMatch
    from unimatch_amd.synth import CONFIGS, synth_state_dict
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    return model.to(DEV).set_precision('exact'), dict(fk)


def _depth_inputs(count, h, w, seed):
    from unimatch_amd.synth import synth_camera, synth_frames
    x = synth_frames(count, h, w, seed=seed) / 255.
    x = (x - torch.tensor((0.485, 0.456, 0.406)).view(1, 3, 1, 1)) / torch.tensor((0.229, 0.224, 0.225)).view(1, 3, 1, 1)
    k, rel = synth_camera(count - 1, h, w)
    return x.contiguous().to(DEV), k.to(DEV), rel.to(DEV)


@pytest.mark.parametrize('bidir', [False, True])
@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_forward_with_depth_confidence(name, bidir):
    from unimatch_amd.ops import KernelTimer
    model, kw = _model(name)
    x, k, rel = _depth_inputs(3, 64, 96, 2300)
    img0, img1 = x[:2].contiguous(), x[1:].contiguous()
    kw = dict(kw, intrinsics=k, pose=rel, pred_bidir_depth=bidir)
    model.launch_parts = 1
    plain = model(img0, img1, **kw)
    assert 'depth_confidence' not in plain
    model.debug_taps = taps = {}
    model.ops.timer = timer = KernelTimer()
    out = model.forward_with_depth_confidence(img0, img1, peak_radius=2, **kw)
    model.ops.timer = None
    model.debug_taps = None
    names = [r[0] for r in timer.records]
    assert names.count('depth_corr_softmax_stats') == 1 and 'depth_corr_softmax' not in names, names
    assert set(out) == set(plain) | {'depth_confidence'} and len(out['flow_preds']) == len(plain['flow_preds'])
    for a, p in zip(out['flow_preds'], plain['flow_preds']):
        print(f'{name} bidir={bidir}: prediction bitwise equal to forward: {torch.equal(a, p)}, max abs {(a - p).abs().max().item():.2e}')
        assert (a - p).abs().max().item() <= TOL * max(1.0, p.abs().max().item())
    conf = out['depth_confidence']
    h, w, d = 8, 12, 64
    assert conf['scale'] == 8 and conf['num_candidates'] == d
    tok0, tok1 = (taps[n].flatten(2).transpose(1, 2).contiguous().cpu().double() for n in ('f0_s0', 'f1_s0'))
    if bidir:
        tok0, tok1 = torch.cat([tok0, tok1], 0), torch.cat([tok1, tok0], 0)
    cam = model.ops.depth_cam(k, rel, 8.0, bidir).cpu()                     # the record the model's launch was given
    assert tuple(cam.shape) == (4 if bidir else 2, 30)
    cand = torch.linspace(kw['min_depth'], kw['max_depth'], d) if 'min_depth' in kw else torch.linspace(1. / 0.5, 1. / 10, d)
    logits, seen = confidence.depth_match_logits_host(tok0, tok1, h, w, cam.double(), cand.double())
    prob = torch.softmax(logits, 1)
    want = confidence.depth_stats_from_prob_host(prob, cand.double(), seen, 2)
    sc = {'max_prob': 1.0, 'peak_mass': 1.0, 'entropy': math.log(d), 'variance': (cand.max() - cand.min()).item() ** 2}
    for key in FLOATS:
        got = conf[key].cpu()
        assert tuple(got.shape) == (4 if bidir else 2, h, w) and got.dtype == torch.float32
        err = (got.double() - getattr(want, key)).abs().max().item()
        print(f'    {key}: {err:.2e} / {TOL * sc[key]:.2e}')
        assert err <= TOL * sc[key], (key, err)
    best = conf['best'].cpu().long()
    assert conf['best'].dtype == torch.int32 and bool((best >= 0).all()) and bool((best < d).all())
    assert (prob.amax(1) - prob.gather(1, best[:, None])[:, 0]).max().item() <= TOL
    clear, gap, _, _ = clear_and_gap(h, w, cam.double(), cand.double(), logits)
    wide = gap >= 0.1
    assert wide.float().mean().item() >= 0.25, wide.float().mean().item()        # the equality clause binds on a real share of the rows
    assert torch.equal(best[wide], prob.argmax(1)[wide])
    assert conf['in_view'].dtype == torch.int32 and clear.float().mean().item() >= 0.95
    assert torch.equal(conf['in_view'].cpu()[clear], want.in_view[clear])
    print(f'    best: wide gap on {wide.float().mean().item():.3f} of the rows; in_view compared on {clear.float().mean().item():.3f}')
    with pytest.raises(NotImplementedError, match='plane sweep'):
        model.forward_with_confidence(img0, img1, **kw)


def test_forward_sequence_depth_confidence_is_taken_in_its_own_forward():
    """``forward_sequence(task='depth', return_confidence=True)``: the depths are within the plane sweep's tolerance of the plain call
    (whose chunks run the plain kernel) and the maps those of the pairwise method (the encoder batch differs: 1e-4 of their range)."""
    model, kw = _model('gmdepth_s1')
    kw.pop('task')
    x, k, rel = _depth_inputs(4, 64, 96, 2301)
    poses = [torch.eye(4, dtype=torch.float64)]
    for i in range(3):
        poses.append(poses[-1] @ torch.linalg.inv(rel[i].cpu().double()))
    poses = torch.stack(poses, 0).float().to(DEV)
    want = model.forward_with_depth_confidence(x[:-1].contiguous(), x[1:].contiguous(), task='depth', intrinsics=k, pose=rel,
                                               **kw)['depth_confidence']
    args = dict(task='depth', intrinsics=k[:1], poses=poses, pairs_per_launch=2, **kw)
    plain = model.forward_sequence(x, **args)
    out = model.forward_sequence(x, return_confidence=True, **args)
    assert 'depth_confidence' not in plain and set(out) == set(plain) | {'depth_confidence'}
    assert (out['depth'] - plain['depth']).abs().max().item() <= TOL * max(1.0, plain['depth'].abs().max().item())
    conf = out['depth_confidence']
    for key in FLOATS:
        assert tuple(conf[key].shape) == (3, 8, 12)
        assert (conf[key] - want[key]).abs().max().item() <= 1e-4 * max(1.0, want[key].abs().max().item()), key
    assert (conf['best'] == want['best']).float().mean() >= 0.95 and (conf['in_view'] == want['in_view']).float().mean() >= 0.95
