"""Inputs and the float64 reference of the multi-view plane-sweep tests (tests/test_depth_multiview_cpu.py, _gpu.py).

The inputs extend those of tests/test_depth_stats_gpu.py: C = 128, ``candidates(d) = linspace(0.1, 2.0, d)``, that file's camera, one
more move ('opposite').  For a tuple of moves the features come from ONE generator seeded ``9001 + 100 h + w``, drawn in this order:
``base = randn(b, C, h, w)``, ``gain = exp(rand(b, 1, h, w) ln(3 / 0.05) + ln 0.05)``, then per source ``f0_s = (base + 0.15 randn) gain``
and ``f1_s = 0.6 base.roll(shift) + 0.4 randn``; everything token-major.  The reference is computed once per case, shared and never
modified."""
import functools
import math

import torch

from unimatch_amd import confidence

C = 128
TOL = 2e-4
DEPTH_BOX = 160               # csrc/local_pixel.h: a (pixel, source) whose corners span more table rows takes the gather form
MOVES = {'sideways': (0.12, -0.01, 0.0), 'diagonal': (0.45, 0.40, 0.0), 'forward': (0.02, 0.01, 0.30), 'away': (15.0, 0.0, 0.0),
         'opposite': (-0.10, 0.02, 0.0)}
SHIFTS = {'sideways': 2, 'opposite': -2, 'diagonal': 3, 'forward': 1, 'away': 0}
FLOATS = ('max_prob', 'entropy', 'variance', 'peak_mass')
# name -> (b, h, w), D, moves
CASES = {'A': ((2, 9, 11), 64, ('sideways', 'opposite')),
         'B': ((2, 16, 24), 64, ('sideways', 'diagonal', 'forward')),        # 'diagonal' mixes box and gather sources in one pixel
         'C': ((2, 16, 24), 80, ('sideways', 'opposite', 'away')),           # the gather kernel, one source that sees nothing
         'D': ((2, 9, 11), 17, ('sideways', 'diagonal')),
         'one1': ((1, 1, 1), 1, ('sideways', 'opposite')),
         'one64': ((1, 1, 1), 64, ('sideways', 'opposite'))}


def candidates(d):
    return torch.linspace(1 / 10.0, 1 / 0.5, d)


def camera(b, h, w, move):
    """The packed ``cam [B, 30]`` float32 of tests/test_depth_stats_gpu.py: fx = 0.9 w, centre (w/2, h/2)."""
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    pose[:, :3, 3] = torch.tensor(MOVES[move])
    if move == 'forward' and b > 1:
        a = 0.04
        pose[1, :3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    return torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous()


@functools.lru_cache(maxsize=None)
def features(b, h, w, moves):
    """Source-major ``f0``, ``f1`` ``[S, B, h*w, 128]`` float32 for the tuple ``moves``."""
    g = torch.Generator().manual_seed(9001 + 100 * h + w)
    base = torch.randn(b, C, h, w, generator=g)
    gain = torch.exp(torch.rand(b, 1, h, w, generator=g) * math.log(3 / 0.05) + math.log(0.05))
    f0, f1 = [], []
    for move in moves:
        f0.append((base + 0.15 * torch.randn(b, C, h, w, generator=g)) * gain)
        f1.append(0.6 * base.roll(SHIFTS[move], dims=-1) + 0.4 * torch.randn(b, C, h, w, generator=g))
    return tuple(torch.stack([f.flatten(2).transpose(1, 2) for f in fs], 0).contiguous() for fs in (f0, f1))


def cameras(b, h, w, moves):
    return torch.stack([camera(b, h, w, m) for m in moves], 0).contiguous()


def inputs(case):
    (b, h, w), d, moves = CASES[case]
    f0, f1 = features(b, h, w, moves)
    return f0, f1, cameras(b, h, w, moves), candidates(d)


def soft_argmin(logits, cand):
    return (torch.softmax(logits, 1) * cand.view(1, -1, 1, 1)).sum(1, keepdim=True)


def reference_of(f0, f1, h, w, cam, cand, use=None, peak_radius=1):
    """float64 of given float32 inputs: the fused logits, prob, statistics, soft-argmin, n_j, and per pixel whether ``in_view`` is
    decided clear of the fp32 rounding of the coordinates of EVERY source that is on, with the gap of the top two logits."""
    f0, f1, cam, cand = f0.double(), f1.double(), cam.double(), cand.double()
    logits, seen, views = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand, use)
    prob = torch.softmax(logits, 1)
    stats = confidence.depth_stats_from_prob_host(prob, cand, seen, peak_radius)
    d = cand.numel()
    clear = torch.ones(logits.shape[0], h, w, dtype=torch.bool)
    for s in range(f0.shape[0]):
        sx, sy = confidence.depth_sample_coords_host(h, w, cam[s], cand)
        near = torch.zeros_like(sx, dtype=torch.bool)
        for coord, hi in ((sx, w), (sy, h)):
            for edge in (-1.0, float(hi)):
                near |= (coord - edge).abs() < 1e-3
        off = torch.zeros(logits.shape[0], dtype=torch.bool) if use is None else ~use[s].bool()
        clear &= ~near.any(1) | off.view(-1, 1, 1)
    top = logits.topk(min(2, d), 1)[0]
    gap = (top[:, 0] - top[:, 1]) if d > 1 else torch.full_like(top[:, 0], float('inf'))
    return dict(logits=logits, prob=prob, stats=stats, out=soft_argmin(logits, cand), views=views, clear=clear, gap=gap)


@functools.lru_cache(maxsize=None)
def reference(case):
    (b, h, w), d, moves = CASES[case]
    f0, f1, cam, cand = inputs(case)
    ref = reference_of(f0, f1, h, w, cam, cand)
    # each single source's prediction and the plain-mean rule's, for the properties of the inputs
    singles, total = [], torch.zeros_like(ref['logits'])
    for s in range(len(moves)):
        lg = confidence.depth_match_logits_host(f0[s].double(), f1[s].double(), h, w, cam[s].double(), cand.double())[0]
        singles.append(soft_argmin(lg, cand.double()))
        total = total + lg
    ref['single_out'] = singles
    ref['plain_mean_out'] = soft_argmin(total / len(moves), cand.double())
    return ref


def box_positions(h, w, cam, cand):
    """Per pixel, the size of the bounding box of one source's corners as the box form computes it (float64 coordinates)."""
    sx, sy = confidence.depth_sample_coords_host(h, w, cam.double(), cand.double())
    x0 = torch.floor(sx).clamp(-1, w - 1)
    y0 = torch.floor(sy).clamp(-1, h - 1)
    return (x0.amax(1) + 1 - x0.amin(1) + 1) * (y0.amax(1) + 1 - y0.amin(1) + 1)


def scales(d):
    cand = candidates(d)
    return {'max_prob': 1.0, 'peak_mass': 1.0, 'entropy': max(1.0, math.log(d)), 'out': cand.max().item(),
            'variance': (cand.max() - cand.min()).item() ** 2}


def check_input_properties():
    """The table of the issue, on the float64 reference: the inputs cannot go soft."""
    share = {}
    for case in 'ABCD':
        ref = reference(case)
        v = ref['views']
        share[case] = [(v == n).double().mean().item() for n in range(4)]
        far = [((ref['out'] - o).abs() > 2e-3).double().mean().item() for o in ref['single_out']]
        assert min(far) >= 0.5, (case, far)
        mean_far = ((ref['out'] - ref['plain_mean_out']).abs() > 2e-3).double().mean().item()
        assert mean_far >= 0.2, (case, mean_far)
        assert ref['logits'].abs().max().item() > 10, (case, ref['logits'].abs().max().item())
    assert share['A'][1] >= 0.05 and share['A'][2] >= 0.5, share['A']
    assert share['B'][1] >= 0.05 and share['B'][3] >= 0.2, share['B']
    assert share['C'][3] == 0, share['C']
    assert share['D'][0] >= 0.03, share['D']
    (b, h, w), d, moves = CASES['B']
    npos = box_positions(h, w, camera(b, h, w, 'diagonal'), candidates(d))
    assert (npos > DEPTH_BOX + 20).any() and (npos < DEPTH_BOX - 20).any(), (npos.min(), npos.max())
    assert (box_positions(h, w, camera(b, h, w, 'sideways'), candidates(d)) < DEPTH_BOX - 20).all()
    return share
