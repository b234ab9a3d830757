"""Cost of the multi-view plane sweep (``um_depth_corr_softmax_multi``) at a user's size: config 5, 480x640 frames, so 60x80 features,
64 candidates, 8 pairs per launch.  Writes ``profiles/depth_multiview.txt``.

  (a) the fused launch at S = 1, 2, 3 against S launches of the two-view ``um_depth_corr_softmax`` on the same operands -- a floor for
      any unfused composition, which would additionally need the logits in HBM;
  (b) the fused launch at S = 1 against the two-view kernel, with the spread of repeating the two-view kernel.

The variants alternate in one process, round after round; a figure is the median over the rounds of the mean over ``--iters`` launches
between two events.  Traffic: the algorithmic bytes from the shapes (every f0 and f1 row of every source once, the outputs once); the
kernels' own traffic needs a counter run, which this tool does not make.

  python tools/bench_depth_multiview.py [--rounds 9] [--iters 20] [--out profiles/depth_multiview.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unimatch_amd.ops import HipOps  # noqa: E402
from unimatch_amd.synth import synth_camera  # noqa: E402

B, H, W, C, D, STRIDE = 8, 60, 80, 128, 64, 8


def operands(sources, dev):
    """Smooth features (a plane sweep's neighbouring candidates land on neighbouring rows, as in a real pair) and the synthetic
    camera's relative poses of consecutive frames, alternating forward / backward neighbours."""
    g = torch.Generator().manual_seed(77)
    base = torch.randn(B, C, H, W, generator=g)
    f0 = torch.stack([(base + 0.15 * torch.randn(B, C, H, W, generator=g)) for _ in range(sources)], 0)
    f1 = torch.stack([0.6 * base.roll(1 + s, -1) + 0.4 * torch.randn(B, C, H, W, generator=g) for s in range(sources)], 0)
    tok = lambda t: t.flatten(3).transpose(2, 3).contiguous().to(dev)
    k, rel = synth_camera(B, H * STRIDE, W * STRIDE)
    k, rel = k.to(dev), rel.to(dev)
    ops = HipOps('exact')
    cams = []
    for s in range(sources):
        pose = rel if s % 2 == 0 else torch.inverse(rel)
        cams.append(ops.depth_cam(k, pose.contiguous(), float(STRIDE)))
    return ops, tok(f0), tok(f1), torch.stack(cams, 0).contiguous(), torch.linspace(1 / 0.5, 1 / 10.0, D, device=dev)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'depth_multiview.txt'))
    args = ap.parse_args()
    dev = 'cuda'
    ops, f0, f1, cam, cand = operands(3, dev)
    h, w = H, W
    variants = {}
    for s in (1, 2, 3):
        a0, a1, ac = f0[:s].contiguous(), f1[:s].contiguous(), cam[:s].contiguous()
        variants[f'fused S={s}'] = (lambda a0=a0, a1=a1, ac=ac: ops.depth_corr_softmax(a0, a1, h, w, ac, cand))
        variants[f'{s} two-view launches'] = (lambda s=s: [ops.depth_corr_softmax(f0[i], f1[i], h, w, cam[i], cand) for i in range(s)])
    variants['two-view again'] = lambda: ops.depth_corr_softmax(f0[0], f1[0], h, w, cam[0], cand)
    for fn in variants.values():                          # warm up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    lines = [f'um_depth_corr_softmax_multi at B={B}, {H}x{W} features, C={C}, D={D} on {torch.cuda.get_device_name(0)}',
             f'{args.rounds} rounds, variants alternating, {args.iters} launches between two events; microseconds per call: median (min .. max)', '']
    for name in variants:
        v = times[name]
        lines.append(f'  {name:24s} {med[name]:9.1f}  ({min(v):.1f} .. {max(v):.1f})')
    lines.append('')
    for s in (1, 2, 3):
        lines.append(f'  (a) fused S={s} / {s} two-view launches: {med[f"fused S={s}"] / med[f"{s} two-view launches"]:.3f}')
    spread = abs(med['two-view again'] - med['1 two-view launches']) / med['1 two-view launches']
    lines.append(f'  (b) fused S=1 / two-view: {med["fused S=1"] / med["1 two-view launches"]:.3f}; '
                 f'the two-view kernel against itself: {med["two-view again"] / med["1 two-view launches"]:.3f} (spread {100 * spread:.1f} %)')
    lines.append('')
    for s in (1, 2, 3):
        algo = s * 2 * B * H * W * C * 4 + B * H * W * 4
        lines.append(f'  algorithmic bytes S={s}: {algo / 1e6:.1f} MB (f0 and f1 of every source once + out); at the fused time '
                     f'{algo / med[f"fused S={s}"] / 1e3:.1f} GB/s')
    lines.append('  (algorithmic bytes only: no counter run was made, so the kernels\' own traffic -- the box rows each pixel re-reads through the')
    lines.append('   caches -- is NOT measured here; profiles/r04_gather_rooflines.txt has the counters of the two-view sweep)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
