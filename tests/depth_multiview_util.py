"""Inputs, the float64 reference and the gates of the multi-view plane-sweep tests (tests/test_depth_multiview_cpu.py, _gpu.py, and
rows 8 .. 11 of tests/test_dispatch_boundaries_cpu.py, _gpu.py).

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
# Rows 8 .. 11 of tests/test_dispatch_boundaries_gpu.py.  Row 8: maps on both sides of the grid cap (GRID_PIXELS), at the box kernel's
# D = 16 and the gather kernel's D = 65; at 2 x 91 x 91 sample 1 starts at pixel 8281, inside a workgroup, and the last 178 pixels are
# on a wave's second trip.  Row 9: four to eight sources ('away' sees nothing, so n_j reaches 7 of 8; a repeated name is another view:
# ``features`` draws fresh noise per source).  Row 11: the gather form's rounds 5 .. 7 with sources that differ.
# On the 128-wide maps D = 16 takes 'forward' where D = 65 has 'opposite': with 'opposite' the 16 coarse candidates leave the largest
# |logit| at 6.46 (128 x 128) and 7.89 (129 x 128), a softmax too flat for the condition |logit|max > 9 of
# tests/test_dispatch_boundaries_cpu.py; with 'forward' it is 9.75 and 10.52 and every other condition of that file holds.
WIDE, WIDE16 = ('sideways', 'opposite', 'diagonal'), ('sideways', 'forward', 'diagonal')
EIGHT = ('sideways', 'opposite', 'diagonal', 'forward', 'away', 'sideways', 'opposite', 'forward')
BOUNDARY = {'cap-1x128x128-d16': ((1, 128, 128), 16, WIDE16), 'cap-1x128x128-d65': ((1, 128, 128), 65, WIDE),
            'cap-1x129x128-d16': ((1, 129, 128), 16, WIDE16), 'cap-1x129x128-d65': ((1, 129, 128), 65, WIDE),
            'cap-2x91x91-d16': ((2, 91, 91), 16, ('sideways', 'opposite', 'forward')),
            'cap-2x91x91-d65': ((2, 91, 91), 65, ('sideways', 'opposite', 'forward')),
            's8-9x11-d17': ((2, 9, 11), 17, EIGHT), 's8-16x24-d64': ((2, 16, 24), 64, EIGHT), 's8-16x24-d80': ((2, 16, 24), 80, EIGHT),
            's5-16x24-d64': ((2, 16, 24), 64, EIGHT[:5]),
            'rounds-d96': ((2, 16, 24), 96, ('sideways', 'diagonal', 'forward')),
            'rounds-d113': ((2, 16, 24), 113, ('sideways', 'opposite', 'forward')),
            'rounds-d128': ((2, 16, 24), 128, ('sideways', 'opposite', 'diagonal'))}
GRID_PIXELS = 4 * 256 * 16    # csrc/local_pixel.h:105-110: 4096 workgroups of 4 waves, one pixel per wave and trip


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


def boundary_geometry(name, masked=False):
    """``(b, h, w), D, moves, use`` of a BOUNDARY case.  ``masked``: a row 8 case ('cap-...') switches source 1 off in its LAST sample
    (the one whose pixels go round again); a row 9 case takes B = 3 and leaves 1, 4 and min(7, S) sources on in samples 0, 1, 2."""
    (b, h, w), d, moves = BOUNDARY[name]
    if not masked:
        return (b, h, w), d, moves, None
    s = len(moves)
    if name.startswith('cap-'):
        use = torch.ones(s, b, dtype=torch.uint8)
        use[1, b - 1] = 0
        return (b, h, w), d, moves, use
    assert s >= 5, name
    use = torch.ones(s, 3, dtype=torch.uint8)
    use[:, 0] = 0
    use[2, 0] = 1                                                # sample 0: 'diagonal' alone
    use[:, 1] = 0
    use[[0, 2, 3, s - 1], 1] = 1                                 # sample 1: four sources
    if s > 7:
        use[1, 2] = 0                                            # sample 2: seven of eight (all five of five)
    return (3, h, w), d, moves, use


def boundary_inputs(name, masked=False):
    (b, h, w), d, moves, use = boundary_geometry(name, masked)
    f0, f1 = features(b, h, w, moves)
    return f0, f1, cameras(b, h, w, moves), candidates(d), use


@functools.lru_cache(maxsize=None)
def boundary_reference(name, masked=False):
    """``reference_of`` a BOUNDARY case (peak_radius 1), computed once, shared, never modified."""
    (b, h, w), d, moves, use = boundary_geometry(name, masked)
    f0, f1, cam, cand, use = boundary_inputs(name, masked)
    return reference_of(f0, f1, h, w, cam, cand, use)


def second_trip(b, h, w):
    """``[b, h, w]`` bool: the pixels a wave reaches on its second trip round the capped grid (``pid >= GRID_PIXELS``)."""
    return (torch.arange(b * h * w) >= GRID_PIXELS).view(b, h, w)


def result_of(ref):
    """``(out, stats [B, 4, h, w], index [B, 2, h, w] int32)`` as a launch returns them, from a float64 reference dict (its ``out``,
    ``stats``): what ``compare`` takes as ``got``.  For the host-side checks that ``compare`` rejects a seeded defect."""
    st = ref['stats']
    return (ref['out'].float(), torch.stack([getattr(st, n) for n in FLOATS], 1).float(),
            torch.stack([st.best.to(torch.int32), st.in_view.to(torch.int32)], 1))


def from_logits(logits, cand, in_view, peak_radius=1):
    """The ``out`` / ``prob`` / ``stats`` entries of a reference dict from given float64 fused logits."""
    prob = torch.softmax(logits, 1)
    return dict(prob=prob, stats=confidence.depth_stats_from_prob_host(prob, cand.double(), in_view, peak_radius),
                out=soft_argmin(logits, cand.double()))


def compare(got, ref, d, label):
    """``got = (out, stats, index)`` of the device against a float64 reference dict, by the gates of tests/test_depth_multiview_gpu.py:
    float planes within ``TOL x scales(d)``, ``best`` by value on every row and by equality where the float64 gap is at least 0.1,
    ``in_view`` equal on the ``clear`` pixels (at least 90 % of the map).  Returns the worst distance per float plane."""
    out, stats, index = (t.cpu() for t in got)
    assert index.dtype == torch.int32 and bool(torch.isfinite(stats).all()) and bool(torch.isfinite(out).all())
    sc = scales(d)
    dist = {'out': (out.double() - ref['out']).abs().max().item()}
    for i, name in enumerate(FLOATS):
        dist[name] = (stats[:, i].double() - getattr(ref['stats'], name)).abs().max().item()
    print(f'{label}: ' + ' '.join(f'{k} {v:.2e}/{TOL * sc[k]:.2e}' for k, v in dist.items()))
    for name, v in dist.items():
        assert v <= TOL * sc[name], (label, name, v, TOL * sc[name])
    best, seen = index[:, 0].long(), index[:, 1]
    assert bool((best >= 0).all()) and bool((best < d).all())
    picked = ref['prob'].gather(1, best[:, None])[:, 0]
    assert (ref['prob'].amax(1) - picked).max().item() <= TOL                      # value optimality: no row excluded
    wide = ref['gap'] >= 0.1
    assert torch.equal(best[wide], ref['prob'].argmax(1)[wide])
    clear = ref['clear']
    assert clear.float().mean().item() >= 0.90, clear.float().mean().item()
    assert torch.equal(seen[clear], ref['stats'].in_view[clear])
    assert bool((seen >= 0).all()) and bool((seen <= d).all())
    return dist


FLIP_GAP = 1e-3               # float64 gap of the top two logits below which fp32 may take the other one as `best`: see compare_about_best


def compare_about_best(got, ref, d, label, peak_radius=1):
    """``compare`` with the reference's ``peak_mass`` taken about the DEVICE's ``best``: the float64 probability within ``peak_radius`` of
    ``got``'s ``best`` plane.  ``peak_mass`` is the one plane that is discontinuous in ``best``, and ``compare`` itself lets ``best`` be
    any candidate whose probability is within TOL of the row maximum, because the top two logits can tie within fp32 rounding.  On maps of
    16384 pixels that happens: at BOUNDARY['cap-1x128x128-d65'] one pixel's top two float64 logits are 4.3e-6 apart, the float32 HOST
    restatement takes the other one, and its ``peak_mass`` is 1.819e-3 from the window about the float64 ``best`` (gate 2e-4) while it
    is exact about its own -- the kernels measured the same 1.819e-3 (tests/test_dispatch_boundaries_cpu.py shows it on the host).
    Where ``best`` agrees with float64 the reference is unchanged, value for value.  ``best`` may differ only where the float64 gap is
    below FLIP_GAP = 1e-3: the fp32 rounding of a logit of magnitude <= 20 out of 128-term dots, a four-corner blend and a mean over up
    to 8 sources stays below 20 x 2^-24 x 140 = 1.7e-4, so two logits further apart than 1e-3 keep their order.  Every other assertion
    is ``compare``'s.  Returns ``compare``'s distances."""
    best = got[2][:, 0].cpu().long()
    flipped = best != ref['stats'].best.long()
    if bool(flipped.any()):
        print(f'{label}: best differs from float64 at {int(flipped.sum())} pixel(s), largest float64 gap there {ref["gap"][flipped].max().item():.2e}')
        assert ref['gap'][flipped].max().item() <= FLIP_GAP, (label, ref['gap'][flipped].max().item())
    j = torch.arange(d).view(1, d, 1, 1)
    about = torch.where((j - best[:, None]).abs() <= int(peak_radius), ref['prob'], torch.zeros_like(ref['prob'])).sum(1)
    assert torch.equal(about[~flipped], ref['stats'].peak_mass[~flipped])
    return compare(got, dict(ref, stats=ref['stats']._replace(peak_mass=about)), d, label)


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
