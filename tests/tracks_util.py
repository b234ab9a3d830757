"""Shared by the point-track tests: an fp64 restatement of the chaining step of ``um_flow_chain`` / ``video.chain_flows`` that also
returns every track's margin to a visibility decision, the seeded smooth inputs, and the acceptance rule of both test files.

The flows are smooth on purpose: a white-noise flow has a gradient of several px/px, which amplifies rounding by that factor at
every step, and no tolerance would then mean anything."""
import torch
import torch.nn.functional as F

from unimatch_amd import video
from unimatch_amd.model import _warp

POS_TOL = 5e-4            # px: half the project's 1e-3 px gate, about 20 x what the float32 paths measure on these inputs
MARGIN_TOL = 1e-3         # a track whose visibility differs from fp64's must be this close to a decision threshold ...
MARGIN_SHARE = 0.01       # ... and at most this share of a case's tracks may be (a condition on the inputs)
# (P, h, w, seed, with mask): dense cases of the CPU and the GPU tests
CASES = ((8, 33, 47, 3, True), (6, 64, 97, 4, True), (12, 48, 64, 5, True), (16, 40, 56, 7, True), (3, 5, 3, 6, False))


def smooth_flows(P, h, w, seed, amp=2.0, drift=(0.75, -0.4)):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(P, 2, 5, 7, generator=g)
    flow = F.interpolate(coarse, (h, w), mode='bilinear', align_corners=True) * amp
    return (flow + torch.tensor(drift).view(1, 2, 1, 1)).float().contiguous()


def backward_flows(fwd, seed):
    """A backward flow that mostly cancels the forward one, with a smooth inconsistency: ``-warp(fwd, -fwd) + noise``."""
    P, _, h, w = fwd.shape
    return (-_warp(fwd, -fwd) + smooth_flows(P, h, w, seed + 100, amp=0.35, drift=(0, 0))).float().contiguous()


_inputs = {}


def inputs(P, h, w, seed, mask=True):
    """``(fwd [P,2,h,w], occ_fwd [P,h,w] or None)`` of a case, made once per session and never written."""
    key = (P, h, w, seed, mask)
    if key not in _inputs:
        fwd = smooth_flows(P, h, w, seed)
        occ = video.forward_backward_consistency_check(fwd, backward_flows(fwd, seed))[0].contiguous() if mask else None
        _inputs[key] = (fwd, occ)
    return _inputs[key]


def sparse_points(h, w, n=257, seed=11):
    """``n`` points: random inside, some outside the frame, some exactly at x = w - 1 / y = h - 1, one NaN.  Returns the points and
    the mask of those that are dead from the start (outside or NaN)."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    pts[:8, 0] = w - 1.0                                   # on the right border: inside
    pts[8:12, 1] = h - 1.0                                 # on the bottom border: inside
    pts[12:16] = torch.tensor([0.0, 0.0])                  # the corner
    pts[16:24, 0] = -0.5 - torch.arange(8.0)               # outside on the left
    pts[24:28, 0] = w - 1.0 + 1e-3                         # just outside on the right
    pts[28:32, 1] = h + 50.0                               # far below
    pts[32, 1] = -1e30
    pts[33, 0] = float('inf')
    pts[40, 0] = float('nan')
    dead = torch.zeros(n, dtype=torch.bool)
    dead[16:34] = True
    dead[40] = True
    return pts.float().contiguous(), dead


def _sample64(planes, x, y):
    c, h, w = planes.shape
    flat = planes.reshape(c, -1)
    x0, y0 = torch.floor(x), torch.floor(y)
    out = torch.zeros(c, x.numel(), dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wt = (1 - (x - xi).abs()) * (1 - (y - yi).abs())
            inb = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)              # false for a NaN
            q = (torch.nan_to_num(yi, nan=0.0).clamp(0, h - 1) * w + torch.nan_to_num(xi, nan=0.0).clamp(0, w - 1)).long()
            out = out + torch.where(inb, wt * flat[:, q], torch.zeros_like(flat[:, q]))
    return out


def chain_fp64(flow, occ=None, points=None, alive=None, stride=1):
    """fp64 restatement -> ``(tracks [P,N,2] float64, visible [P,N] bool, margin [N] float64)``.  The margin is the minimum, over the
    steps a track is alive at, of the new position's distance to the nearest frame border and of ``|o - 0.5|``: how far the track
    stayed from a visibility decision that rounding could flip (inf for a track that never was alive)."""
    P, _, h, w = flow.shape
    flow = flow.double()
    occ = None if occ is None else occ.double()
    if points is None:
        points = video.start_grid(h, w, stride)
    x, y = points[:, 0].double().clone(), points[:, 1].double().clone()

    def inside(x, y):
        return (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    live = inside(x, y) if alive is None else alive & inside(x, y)
    margin = torch.full_like(x, float('inf'))
    tracks, visible = [], []
    for t in range(P):
        uv = _sample64(flow[t], x, y)
        nx, ny = torch.where(live, x + uv[0], x), torch.where(live, y + uv[1], y)
        m = torch.minimum(torch.minimum(nx, w - 1 - nx), torch.minimum(ny, h - 1 - ny)).abs()
        still = live & inside(nx, ny)
        if occ is not None:
            o = _sample64(occ[t][None], x, y)[0]
            still = still & ~(o >= 0.5)
            m = torch.minimum(m, (o - 0.5).abs())
        margin = torch.where(live, torch.minimum(margin, torch.nan_to_num(m, nan=0.0)), margin)
        x, y, live = nx, ny, still
        tracks.append(torch.stack([x, y], -1))
        visible.append(live)
    return torch.stack(tracks, 0), torch.stack(visible, 0), margin


def accept(tracks, visible, want):
    """The acceptance rule.  ``want`` is :func:`chain_fp64`'s result for the same inputs.  Returns the largest position distance (px)
    on the tracks whose visibility rows agree."""
    t64, v64, margin = want
    tracks, visible = tracks.cpu(), visible.cpu()
    assert tracks.dtype == torch.float32 and visible.dtype == torch.bool
    assert tuple(tracks.shape) == tuple(t64.shape) and tuple(visible.shape) == tuple(v64.shape)
    near = margin < MARGIN_TOL
    assert near.float().mean().item() <= MARGIN_SHARE, ('inputs too close to a threshold', near.float().mean().item())
    agree = (visible == v64).all(0)
    assert (near[~agree]).all(), ('visibility differs away from a threshold', int((~agree & ~near).sum()), margin[~agree].max().item())
    both = agree & torch.isfinite(t64).all(-1).all(0)                  # a NaN / inf start stays what it is: compared separately
    err = (tracks.double() - t64).abs().amax(-1)[:, both]
    worst = err.max().item() if err.numel() else 0.0
    assert worst <= POS_TOL, worst
    odd = agree & ~both
    assert torch.equal(torch.nan_to_num(tracks[:, odd], nan=7.0, posinf=8.0, neginf=9.0),
                       torch.nan_to_num(t64[:, odd].float(), nan=7.0, posinf=8.0, neginf=9.0))
    return worst


def check_composition(tracks, visible, comp, h, w):
    """``tracks`` against the reference's composition plus the start grid, on every (track, step) where the track was alive BEFORE
    the step: once a track has left the frame the reference goes on adding zeros, so it is not the definition there."""
    P = comp.shape[0]
    want = comp.permute(0, 2, 3, 1).reshape(P, h * w, 2) + video.start_grid(h, w)
    before = torch.cat([torch.ones(1, h * w, dtype=torch.bool), visible[:-1].cpu()], 0)
    share = before.float().mean().item()
    worst = (tracks.cpu() - want).abs().amax(-1)[before].max().item()
    print(f'composition {P}x{h}x{w}: max |d| {worst:.3e} px over {share:.1%} of the entries')
    assert share >= 0.75, share
    assert worst <= 1e-4, worst
