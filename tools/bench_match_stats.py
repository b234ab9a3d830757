"""Cost of the matching-confidence launch next to the matching launch it rides beside, and next to what a caller had before it.

    python tools/bench_match_stats.py [--out profiles/match_stats.txt] [--batch 8] [--height 64] [--width 96]

The size is config 2's matching size: B = 8 at 64 x 96 (6144 tokens), exact and fast mode.  Three legs on the same inputs:

  stats    ``um_global_match_stats`` (``confidence.global_match_stats``): planes, one match_stats_kernel launch
  match    ``um_global_corr_softmax_flow`` (``HipOps.global_corr_softmax_flow``): planes, the fused matching launch
  torch    the baseline a caller has today: torch ops on the GPU that form ``prob`` [B, L, L] and reduce it
           (``confidence.global_match_stats_host`` on CUDA float32 tensors, one sample at a time: 151 MB of ``prob`` per sample)

The legs alternate inside one process after a warm-up of each; a region is as many calls as last at least 0.5 s, timed with device
events; the figure is the median of the regions.  The file also records the distances of the GPU test's cases to float64 next to
the float32 host restatement's and the test's floors (``tests/test_match_stats_gpu.py``), and the compiler's resource report of the
kernel.
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import confidence  # noqa: E402
from unimatch_amd.ops import HipOps  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 5
REGION_SECONDS = 0.5
MFMA_PEAK = {'exact': 2.5e15 / 3, 'fast': 2.5e15}          # dense fp16 / bf16 FLOP/s of an MI355X; exact mode spends three products


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
    for _ in range(REGIONS):
        for k, fn in fns.items():
            times[k].append(timed(fn, calls[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, calls


def resource_report():
    path = os.path.join(ROOT, 'unimatch_amd', '_obj', 'match_stats.resources.txt')
    if not os.path.exists(path):
        return ['  (no resource report next to the library: build with `python -m unimatch_amd.build`)']
    out, name = [], None
    keep = ('VGPRs:', 'AGPRs:', 'ScratchSize', 'Occupancy', 'LDS Size')
    for ln in open(path):
        if 'Function Name:' in ln:
            name = ln.split('Function Name:')[1].split()[0]
            if 'match_stats_kernel' in name:
                out.append(f'  {name}')
        elif name and 'match_stats_kernel' in name and any(k in ln for k in keep):
            out.append('      ' + ln.split('remark:')[1].split('[-R')[0].strip())
    return out


def parity_lines():
    """The GPU test's cases: kernel and float32-host distances to float64, and the floors."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from tests import test_match_stats_gpu as t
    lines = ['distance to float64 (max abs) per case: kernel | float32 host restatement | floor | bound = 2 x host + floor']
    for precision in ('exact', 'fast'):
        for kind, b, h, w in t.CASES:
            stereo = kind == 'stereo'
            f0, f1, _, r64, r32, _, _ = t.reference(kind, b, h, w, precision)
            got = confidence.global_match_stats(f0.cuda(), f1.cuda(), h, w, stereo=stereo, precision=precision)
            fl = t.floors(h, w, stereo)
            for name in t.FIELDS:
                d = (getattr(got, name).double().cpu() - getattr(r64, name)).abs().max().item()
                d32 = (getattr(r32, name).double() - getattr(r64, name)).abs().max().item()
                lines.append(f'  {precision:<6}{kind:<10}{b}x{h}x{w:<5}{name:<9} {d:9.2e} | {d32:9.2e} | {fl[name]:9.2e} | {2 * d32 + fl[name]:9.2e}'
                             f'{"" if d <= 2 * d32 + fl[name] else "   OVER"}')
    return lines


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: this is a measurement, there is no fallback')
    b, h, w = arg('--batch', 8), arg('--height', 64), arg('--width', 96)
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'match_stats.txt'))
    l, c = h * w, 128
    g = torch.Generator().manual_seed(3)
    f0 = torch.randn(b, l, c, generator=g).cuda()
    f1 = (f0[:, torch.randperm(l, generator=g)] * 0.5 + 0.5 * torch.randn(b, l, c, generator=g).cuda()).contiguous()
    lines = [f'matching confidence at B = {b}, {h} x {w} ({l} tokens), {torch.cuda.get_device_name(0)}', '']

    def torch_leg():
        return [confidence.global_match_stats_host(f0[i:i + 1], f1[i:i + 1], h, w) for i in range(b)]

    stats_time = {}
    for precision in ('exact', 'fast'):
        ops = HipOps(precision)
        t, calls = alternate({'stats': lambda: confidence.global_match_stats(f0, f1, h, w, precision=precision),
                              'match': lambda: ops.global_corr_softmax_flow(f0, f1, h, w),
                              'torch': torch_leg})
        lines.append(f'{precision} mode, microseconds per call (median of {REGIONS} regions of >= {REGION_SECONDS} s, [min .. max])')
        for k, (med, lo, hi) in t.items():
            lines.append(f'  {k:<6}{med * 1e6:11.1f} us  [{lo * 1e6:.1f} .. {hi * 1e6:.1f}]   {calls[k]} calls per region')
        stats_time[precision] = t['stats'][0]
        flops = 2.0 * b * l * l * c
        lines.append(f'  stats / match {t["stats"][0] / t["match"][0]:7.2f} x      torch / stats {t["torch"][0] / t["stats"][0]:7.2f} x')
        lines.append(f'  stats: {flops / t["stats"][0] / 1e12:.0f} TFLOP/s of useful products, {100 * flops / t["stats"][0] / MFMA_PEAK[precision]:.0f} % '
                     f'of what the matrix cores could do in this mode')
        if t['stats'][0] > t['match'][0]:
            lines.append('  the stats launch costs more than the matching launch (what bounds it: DESIGN.md 7f, with the resource report below)')
        lines.append('')
        print('\n'.join(lines[-8:]), flush=True)
    lines += [f'fast / exact time of the stats launch: {stats_time["fast"] / stats_time["exact"]:.2f} (a third of the MFMA products)', '']
    lines += ['compiler resource report (match_stats_kernel<operand type, planes, causal>)'] + resource_report() + ['']
    lines += parity_lines()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-60:]))
    print('written', out_path)


if __name__ == '__main__':
    main()
