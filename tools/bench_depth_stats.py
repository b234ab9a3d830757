"""Cost of the plane sweep with statistics (``um_depth_corr_softmax_stats``) next to the plain sweep, before and after the change.

    python tools/bench_depth_stats.py [--parent-lib PATH] [--parent-resources PATH] [--out profiles/depth_match_stats.txt]

The size is the depth configuration's matching step: 480 x 640 images, 60 x 80 features, B = 16 pairs, D = 64 inverse-depth candidates
(the box kernel), ScanNet intrinsics over the feature stride and ``synth_camera``'s relative pose.  Three legs on the same inputs:

  parent   ``um_depth_corr_softmax`` of a library built from the parent commit (``--parent-lib``: check the parent out into a
           worktree, ``python -m unimatch_amd.build`` there, pass its ``libunimatch_hip.so``); left out when no library is given
  plain    ``um_depth_corr_softmax`` of this tree's library
  fused    ``um_depth_corr_softmax_stats`` of this tree's library: the prediction, four statistics planes and two index planes

A RUN is a fresh process (the tool starts itself ``--runs`` times, one after the other): in it the legs alternate after a warm-up of
each, in an order that rotates from region to region; a region is as many calls as last at least 0.5 s, timed with device events, and
the run's figure is the median of its regions.  The file gives, per leg, the median over the runs and the run-to-run spread
[min .. max].  Two conditions are evaluated and written down, neither against a number fixed in advance: the plain kernel stays
within the parent's own run-to-run spread, and the fused launch costs less than two plain launches (otherwise fusing bought nothing
over a second sweep).  The file also records the compiler's resource report of the K7 kernels (``--parent-resources``: the parent's report, from the same compile line) and the distances of the
GPU test's cases to float64 next to their gates: the cases, inputs and float64 reference are imported from
``tests/test_depth_stats_gpu.py`` (the tool depends on that test module, so that the file reports exactly what the test gates).
"""
import ctypes
import json
import math
import os
import subprocess
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import _abi  # noqa: E402
from unimatch_amd.synth import synth_camera  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 6
RUNS = 5
REGION_SECONDS = 0.5
RUN_TIMEOUT = 120            # seconds per run: start-up, three warm-ups and 3 x REGIONS regions take about 15
C = 128


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / calls


def alternate(fns):
    calls = {}
    for k, fn in fns.items():
        timed(fn, 3)
        calls[k] = max(1, int(REGION_SECONDS / timed(fn, 3)) + 1)
    times = {k: [] for k in fns}
    order = list(fns)
    for r in range(REGIONS):
        for k in order[r % len(order):] + order[:r % len(order)]:          # no leg always follows the same other leg
            times[k].append(timed(fns[k], calls[k]))
    return {k: statistics.median(v) for k, v in times.items()}, calls


def resource_lines(path, title):
    if not path or not os.path.exists(path):
        return [f'{title}: no resource report given']
    out, name = [title], None
    keep = ('VGPRs:', 'TotalSGPRs:', 'ScratchSize', 'Occupancy', 'LDS Size')
    for ln in open(path):
        if 'Function Name:' in ln:
            name = ln.split('Function Name:')[1].split()[0]
            if 'depth_corr_softmax' in name:
                out.append(f'  {name}')
        elif name and 'depth_corr_softmax' in name and any(k in ln for k in keep):
            out.append('      ' + ln.split('remark:')[1].split('[-R')[0].strip())
    return out


def parity_lines():
    """The GPU test's cases against float64: max abs distance per output over its gate (2e-4 x scale), and the index planes."""
    from tests import test_depth_stats_gpu as t
    from unimatch_amd.ops import HipOps
    ops = HipOps('exact')
    lines = ['distance to float64 (max abs) / gate per case of tests/test_depth_stats_gpu.py; best: share of rows equal to the float64 arg-max '
             '(share with a float64 gap >= 0.1, where equality is required); in_view: share equal on the compared pixels (share compared)']
    worst = {}
    for b, h, w in t.SHAPES:
        for d in t.COUNTS:
            for move in t.MOVES:
                ref = t.reference(b, h, w, d, move)
                out, stats, index = (x.cpu() for x in t.launch(ops, b, h, w, d, move))
                sc = t.scales(d)
                dist = {'out': (out.double() - ref['out']).abs().max().item()}
                for i, name in enumerate(t.FLOATS):
                    dist[name] = (stats[:, i].double() - getattr(ref['stats'], name)).abs().max().item()
                for k, v in dist.items():
                    if sc[k] > 0:                                         # one candidate: the variance's scale is 0 and so is the variance
                        worst[k] = max(worst.get(k, 0.0), v / (t.TOL * sc[k]))
                best = index[:, 0].long()
                same = (best == ref['prob'].argmax(1)).float().mean().item()
                clear = ref['clear']
                seen = (index[:, 1][clear] == ref['stats'].in_view[clear]).float().mean().item() if bool(clear.any()) else float('nan')
                lines.append(f'  {b}x{h}x{w:<3} D={d:<4}{move:<9} ' + ' '.join(f'{k} {v:.1e}/{t.TOL * sc[k]:.1e}' for k, v in dist.items())
                             + f'  best {same:.3f} ({(ref["gap"] >= 0.1).float().mean().item():.3f})  in_view {seen:.3f} ({clear.float().mean().item():.3f})')
    lines.append('  largest distance over its gate, per output: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    f0, f1 = (f.cuda() for f in t.features(2, 16, 24))
    for d, move in ((64, 'sideways'), (64, 'diagonal'), (128, 'forward')):
        cam, cand = t.camera(2, 16, 24, move).cuda(), t.candidates(d).cuda()
        same = torch.equal(ops.depth_corr_softmax(f0, f1, 16, 24, cam, cand), ops.depth_corr_softmax(f0, f1, 16, 24, cam, cand, stats=True)[0])
        lines.append(f'  fused out bitwise equal to the plain kernel at 2x16x24 D={d} {move}: {same}')
    return lines


def one_run(b, h, w, d, parent_path):
    """One run, in this process: ``{'seconds': {leg: median}, 'calls': {leg: per region}, 'same': parent and plain outputs equal}``."""
    g = torch.Generator().manual_seed(5)
    m0 = torch.randn(b, C, h, w, generator=g)
    m1 = 0.6 * m0.roll(2, dims=-1) + 0.4 * torch.randn(b, C, h, w, generator=g)
    m0 = m0 * torch.exp(torch.rand(b, 1, h, w, generator=g) * math.log(3 / 0.05) + math.log(0.05))
    f0, f1 = (m.flatten(2).transpose(1, 2).contiguous().cuda() for m in (m0, m1))
    k, pose = synth_camera(b, 8 * h, 8 * w)
    k[:, :2] = k[:, :2] / 8
    cam = torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous().cuda()
    cand = torch.linspace(1 / 10.0, 1 / 0.5, d).cuda()
    out = torch.empty((b, 1, h, w), device='cuda')
    stats = torch.empty((b, 4, h, w), device='cuda')
    index = torch.empty((b, 2, h, w), dtype=torch.int32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    lib = _abi.load()
    ptrs = [t.data_ptr() for t in (f0, f1, cam, cand, out)]

    def plain_of(library):
        return lambda: _abi.check(library.um_depth_corr_softmax(*ptrs, b, h, w, C, d, 0, stream), 'um_depth_corr_softmax')

    legs = {}
    if parent_path:
        parent = ctypes.CDLL(os.path.abspath(parent_path))
        if hasattr(parent, 'um_depth_corr_softmax_stats'):
            raise SystemExit(f'{parent_path} already has um_depth_corr_softmax_stats: it is not the parent commit\'s library')
        parent.um_depth_corr_softmax.restype, parent.um_depth_corr_softmax.argtypes = _abi.SIGNATURES['um_depth_corr_softmax']
        legs['parent'] = plain_of(parent)
    legs['plain'] = plain_of(lib)
    legs['fused'] = lambda: _abi.check(lib.um_depth_corr_softmax_stats(*ptrs, stats.data_ptr(), index.data_ptr(), b, h, w, C, d, 0, 1, stream),
                                       'um_depth_corr_softmax_stats')
    same = None
    if parent_path:                                       # the same kernel on the same inputs: the results must be the same bytes
        legs['parent']()
        before = out.clone()
        legs['plain']()
        same = torch.equal(before, out)
    t, calls = alternate(legs)
    return {'seconds': t, 'calls': calls, 'same': same}


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: this is a measurement, there is no fallback')
    b, h, w, d = arg('--batch', 16), arg('--height', 60), arg('--width', 80), arg('--candidates', 64)
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'depth_match_stats.txt'))
    parent_path, parent_res = arg('--parent-lib', ''), arg('--parent-resources', '')
    if '--one-run' in ARGV:                               # a child: one run's medians as a JSON line
        print('RUN ' + json.dumps(one_run(b, h, w, d, parent_path)), flush=True)
        return
    runs = []
    for _ in range(arg('--runs', RUNS)):                  # one after the other, each a fresh process; this one launches nothing meanwhile
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--one-run'] + ARGV, stdout=subprocess.PIPE, text=True, check=True,
                              timeout=RUN_TIMEOUT)            # a run that hangs ends the tool (TimeoutExpired) instead of hanging it
        runs.append(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('RUN ')][-1][4:]))
        print({k: round(v * 1e6, 2) for k, v in runs[-1]['seconds'].items()}, flush=True)
    t = {k: (statistics.median(r['seconds'][k] for r in runs), min(r['seconds'][k] for r in runs), max(r['seconds'][k] for r in runs))
         for k in runs[0]['seconds']}
    calls, same = runs[0]['calls'], all(r['same'] for r in runs) if parent_path else None
    lines = [f'plane sweep with statistics at B = {b}, {h} x {w} features ({8 * h} x {8 * w} images), D = {d}, {torch.cuda.get_device_name(0)}', '',
             f'microseconds per call: median over {len(runs)} runs (fresh processes; a run is the median of {REGIONS} alternating regions of '
             f'>= {REGION_SECONDS} s), [min .. max] over the runs']
    for name, (med, lo, hi) in t.items():
        lines.append(f'  {name:<7}{med * 1e6:10.1f} us  [{lo * 1e6:.1f} .. {hi * 1e6:.1f}]   {calls[name]} calls per region')
    plain, fused = t['plain'][0], t['fused'][0]
    lines.append('')
    if parent_path:
        med, lo, hi = t['parent']
        inside = lo <= plain <= hi
        lines += [f'plain at this commit / at the parent: {plain / med:.4f}; the parent\'s own runs spread {100 * (hi - lo) / med:.2f} % '
                  f'of its median ({lo * 1e6:.1f} .. {hi * 1e6:.1f} us)',
                  f'  condition 1, the plain kernel stays within the parent\'s run-to-run spread: {"holds" if inside else "DOES NOT HOLD"} '
                  f'(median {plain * 1e6:.1f} us); outputs of the two libraries bitwise equal: {same}']
    else:
        lines.append('parent: not measured (no --parent-lib given)')
    lines += [f'fused / plain: {fused / plain:.3f}',
              f'  condition 2, the fused launch costs less than two plain launches: {"holds" if fused < 2 * plain else "DOES NOT HOLD"} '
              f'({fused * 1e6:.1f} us against {2 * plain * 1e6:.1f} us)', '']
    print('\n'.join(lines), flush=True)
    lines += resource_lines(parent_res, 'compiler resource report, K7 at the parent commit') + ['']
    lines += resource_lines(os.path.join(ROOT, 'unimatch_amd', '_obj', 'local_ops.resources.txt'),
                            'compiler resource report, K7 at this commit (*_stats_kernel: um_depth_corr_softmax_stats)') + ['']
    lines += parity_lines()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-90:]))
    print('written', out_path)


if __name__ == '__main__':
    main()
