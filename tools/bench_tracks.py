"""Point tracks: ``um_flow_chain`` (one launch per chunk, the state in registers) against the loop of torch ops a caller writes
without it -- per step: add the grid, normalise, ``grid_sample`` of the flow and of the mask, threshold, ``where``.

    python tools/bench_tracks.py [--out profiles/tracks.txt] [--region 0.25]

Rows: dense 512 x 768 and 720 x 1280 with P = 8 pairs, and 4096 sparse points at 512 x 768.  Both legs get the same smooth flows
(bilinear upsampling of a 1/32 noise grid, as predicted flows are; the backward flow is the warped negative plus a smooth
inconsistency, so that most tracks live through the chunk) and the masks of ``um_fwd_bwd_occlusion``.  The legs alternate in one
process; each is timed as a synchronised region (synchronize, wall clock, synchronize) of as many back-to-back chunks as fill
``--region`` seconds, the median of 3 regions per leg is reported as ms per chunk.  GB/s is the algorithmic traffic ``P (12 B read + 9 B written)`` per track -- the floor:
a flow sample (8 B) and a mask sample (4 B) from cached lines, a position (8 B) and a flag (1 B) out -- over that time.  The largest
distance between the kernel and an fp64 run of the host restatement is recorded too (tracks whose visibility rows agree).
"""
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import video  # noqa: E402
from unimatch_amd.model import _warp  # noqa: E402

ARGV = sys.argv[1:]


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns, reps=3):
    """Median wall time of each callable over ``reps`` synchronised regions, the callables alternating."""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(region(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def smooth(p, h, w, seed, rms):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(p, 2, h // 32, w // 32, generator=g) * rms
    return F.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True).contiguous()


def op_loop(flow, occ, points):
    """The host-side loop over torch ops: ``points [N, 2]`` -> (tracks [P, N, 2], visible [P, N])."""
    p, _, h, w = flow.shape
    scale = torch.tensor([2.0 / (w - 1), 2.0 / (h - 1)], device=flow.device)
    hi = torch.tensor([w - 1.0, h - 1.0], device=flow.device)
    pos = points.clone()
    alive = ((pos >= 0) & (pos <= hi)).all(-1)
    tracks, visible = [], []
    for t in range(p):
        grid = (pos * scale - 1.0).view(1, 1, -1, 2)
        uv = F.grid_sample(flow[t:t + 1], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0, :, 0].t()
        o = F.grid_sample(occ[t:t + 1, None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0, 0, 0]
        moved = pos + uv
        pos = torch.where(alive[:, None], moved, pos)
        alive = alive & ((pos >= 0) & (pos <= hi)).all(-1) & ~(o >= 0.5)
        tracks.append(pos)
        visible.append(alive)
    return torch.stack(tracks, 0), torch.stack(visible, 0)


def row(name, p, h, w, points, seconds):
    fwd = (smooth(p, h, w, 1, 3.0) + torch.tensor([1.5, -0.75]).view(1, 2, 1, 1)).cuda()
    bwd = -_warp(fwd, -fwd) + smooth(p, h, w, 2, 0.22).cuda()
    occ = video.forward_backward_consistency_check(fwd, bwd)[0]
    start = video.start_grid(h, w, device='cuda') if points is None else points.cuda()
    n = start.shape[0]

    calls = {'kernel': lambda: video.chain_flows(fwd, occ, points=None if points is None else start),
             'ops': lambda: op_loop(fwd, occ, start)}

    def repeat(fn, count):
        for _ in range(count):
            fn()

    inner = {}
    for k, fn in calls.items():                        # warm up, then size the region from a short one
        repeat(fn, 3)
        inner[k] = max(5, int(seconds / (region(lambda: repeat(fn, 10)) / 10)))
    t = alternate({k: (lambda k=k: repeat(calls[k], inner[k])) for k in calls})
    tk, vk = video.chain_flows(fwd, occ, points=None if points is None else start)
    to, vo = op_loop(fwd, occ, start)
    t64, v64 = video._chain_flows_host(fwd.cpu().double(), occ.cpu().double(), start.cpu().double(), torch.ones(n, dtype=torch.bool))
    agree = (vk.cpu() == v64).all(0)
    dist = (tk.cpu().double() - t64).abs().amax(-1)[:, agree].max().item()
    same = (vk == vo).all(0)
    dops = (tk - to).abs().amax(-1)[:, same].max().item()
    traffic = p * 21.0 * n
    ms = {k: 1e3 * v / inner[k] for k, v in t.items()}
    lines = [f'{name}: P = {p}, {h} x {w}, N = {n} tracks, occluded {occ.mean().item():.1%}, alive at the end {vk[-1].float().mean().item():.1%}',
             f'  um_flow_chain     {ms["kernel"]:9.4f} ms per chunk   {traffic / (ms["kernel"] * 1e-3) / 1e9:9.1f} GB/s of the {traffic / 1e6:.2f} MB floor'
             f'   ({inner["kernel"]} chunks per region)',
             f'  torch-op loop     {ms["ops"]:9.4f} ms per chunk   {traffic / (ms["ops"] * 1e-3) / 1e9:9.1f} GB/s   ({inner["ops"]} chunks per region)',
             f'  op loop / kernel  {ms["ops"] / ms["kernel"]:9.2f} x   ({"the kernel is faster" if ms["kernel"] < ms["ops"] else "the kernel is NOT faster"})',
             f'  kernel vs fp64 restatement: max |d| {dist:.3e} px on the {agree.float().mean().item():.3%} of tracks whose visibility agrees',
             f'  kernel vs op loop:          max |d| {dops:.3e} px on the {same.float().mean().item():.3%} of tracks whose visibility agrees']
    print('\n'.join(lines), flush=True)
    return lines


def main():
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'tracks.txt'))
    seconds = arg('--region', 0.25)
    g = torch.Generator().manual_seed(3)
    sparse = torch.rand(4096, 2, generator=g) * torch.tensor([767.0, 511.0])
    lines = [f'tools/bench_tracks.py on {torch.cuda.get_device_name(0)}: median of 3 synchronised regions of about {seconds} s per leg, '
             'legs alternated', '']
    for name, p, h, w, pts in (('dense', 8, 512, 768, None), ('dense', 8, 720, 1280, None), ('sparse', 8, 512, 768, sparse)):
        lines += row(name, p, h, w, pts, seconds) + ['']
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines))


if __name__ == '__main__':
    main()
