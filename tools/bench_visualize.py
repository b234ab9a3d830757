"""Cost of colouring a disparity or depth prediction: the host path the reference takes against the device path.

    python tools/bench_visualize.py [--out profiles/visualize.txt] [--iters 10]

Two images, each at 480 x 640 and 1080 x 1920, batch 1 and batch 8; the prediction is on the device in every leg, as the model
leaves it, and the coloured uint8 image ends on the host in every leg, where a runner writes it to a file:

  disparity      vis_disparity: min-max normalisation, 8-bit index, inferno
  inverse depth  viz_depth_tensor(1 / depth): minimum to 95th percentile, plasma

  host    ``pred.cpu()`` (4 bytes per pixel over the bus), then the NumPy restatement of ``unimatch_amd.visualize`` (for the inverse
          depth: a full sort per image)
  device  ``um_scalar_to_rgb`` (for the inverse depth: the three-digit radix select), then ``rgb.cpu()`` (3 bytes per pixel)
  kernel  the device leg without the copy back: the launches alone

Every figure is the median of 7 synchronised regions of ``--iters`` calls (synchronize, wall clock, synchronize) after a warm-up of
every leg, the legs alternating inside one process; the spread is (max - min) / median over the regions.  Nobody had measured these
before: both columns are recorded whatever the ratio, and a size at which the device path loses is marked as such.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import visualize  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 7


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def region(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def alternate(fns, iters, regions=REGIONS):
    for fn in fns.values():                            # warm-up of every leg
        fn()
    times = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            times[k].append(region(fn, iters))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in times.items()}


def smooth(b, h, w, lo, hi, seed):
    """A smooth field plus a little noise in ``[lo, hi]``: what a prediction looks like (long runs of one exponent)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b, 1, h // 16, w // 16, generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True)[:, 0]
    field = (field + 0.02 * torch.rand(b, h, w, generator=g)) / 1.02
    return (lo + (hi - lo) * field).float().contiguous()


def rows(kind, b, h, w, iters, lines):
    if kind == 'disparity':
        x, fn = smooth(b, h, w, 0.5, 192.0, 1).cuda(), visualize.disparity_to_image
    else:
        x, fn = smooth(b, h, w, 0.5, 10.0, 2).cuda(), visualize.inverse_depth_to_image
    assert torch.equal(fn(x).cpu(), fn(x.cpu()))       # the two paths give the same image
    legs = {'host': lambda: fn(x.cpu()), 'device': lambda: fn(x).cpu(), 'kernel': lambda: fn(x)}
    t = alternate(legs, max(1, iters // 4) if h * w * b > 4e6 else iters)
    lines.append(f'{kind}, batch {b}, {h} x {w} (ms per call: median, spread over {REGIONS} regions)')
    for k, (med, spread) in t.items():
        lines.append(f'  {k:<8}{1e3 * med:10.4f}   spread {100 * spread:5.1f} %')
    allow = max(t['host'][1], t['device'][1])
    verdict = 'not slower' if t['device'][0] <= t['host'][0] * (1 + allow) else 'SLOWER: the device path loses here'
    lines.append(f'  host / device {t["host"][0] / t["device"][0]:8.2f} x   -> the device path is {verdict} (allowance: the spread, {100 * allow:.1f} %)')
    lines.append('')
    print('\n'.join(lines[-6:]), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'visualize.txt'))
    iters = arg('--iters', 10)
    lines = [f'tools/bench_visualize.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'median of {REGIONS} synchronised regions of {iters} calls per leg (a quarter of that above 4 Mpx), legs alternating in one '
             'process, every leg warmed up once',
             'host = copy the prediction back, NumPy recipe; device = um_scalar_to_rgb, copy the image back; kernel = um_scalar_to_rgb alone',
             '']
    for kind in ('disparity', 'inverse depth'):
        for h, w in ((480, 640), (1080, 1920)):
            for b in (1, 8):
                rows(kind, b, h, w, iters, lines)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
