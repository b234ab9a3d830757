"""Cost of the fused sequence mode of posed-video depth (``forward_sequence(task='depth', fuse_neighbours=True)``).  Writes
``profiles/depth_fuse_neighbours.txt``.

  (a) the row-table launch (``um_depth_corr_softmax_multi_rows``) on a chunk's operands where the Transformer left them -- tok0 [8],
      tok1 [8] and the carried pair [2], B = 8, 60x80 features, D = 64, S = 2 -- against materialising the source-major operands with
      ``torch.cat`` / ``torch.stack`` and launching the contiguous ``um_depth_corr_softmax_multi`` on them, against that contiguous
      launch alone (its operands ready: a floor no sequence chunk reaches), and against the row-table launch again (the run's spread);
  (b) ms per depth map on ``--frames`` frames of 480x640 at 1, 4 and 8 pairs per launch: the sequence mode unfused, with
      ``pred_bidir_depth``, fused, and the per-frame ``forward_multiview`` loop the fused mode replaces (which has no chunks).

Protocol of tools/bench_depth_multiview.py and tools/bench_depth_sequence.py: the variants alternate in one process, round after round,
after two warm-up rounds; (a) is the mean over ``--iters`` launches between two events, (b) the wall time of ``--passes`` runs of the video
between two device synchronisations; a figure is the median over the rounds with min .. max.

  python tools/bench_depth_fuse_neighbours.py [--rounds 9] [--iters 20] [--frames 33] [--reps 5] [--passes 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import UniMatch  # noqa: E402
from unimatch_amd.model import neighbour_rows  # noqa: E402
from unimatch_amd.ops import HipOps  # noqa: E402
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_frames, synth_state_dict  # noqa: E402

B, H, W, C, D, STRIDE = 8, 60, 80, 128, 64, 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters          # microseconds per call


def fmt(v, scale=1.0, digits=1):
    return f'{scale * statistics.median(v):9.{digits}f}  ({scale * min(v):.{digits}f} .. {scale * max(v):.{digits}f})'


def launch_part(args, dev):
    """(a): the operands of one chunk of 8 consecutive pairs behind a carried pair, as ``_match`` holds them."""
    g = torch.Generator().manual_seed(78)
    base = torch.randn(B + 1, C, H, W, generator=g)
    tok = lambda t: t.flatten(2).transpose(1, 2).contiguous().to(dev)
    # pair t = frames (t - 1, t) of B + 2 frames; tok0 / tok1: smooth features, neighbouring candidates land on neighbouring rows
    all0 = tok(base + 0.15 * torch.randn(B + 1, C, H, W, generator=g))
    all1 = tok(0.6 * base.roll(1, -1) + 0.4 * torch.randn(B + 1, C, H, W, generator=g))
    carried = torch.stack([all0[0], all1[0]], 0).contiguous()
    stream = torch.cat([all0[1:], all1[1:]], 0).contiguous()           # the Transformer's output: tok0 and tok1 are its two halves
    tok0, tok1 = stream[:B], stream[B:]
    k, rel = synth_camera(B + 1, H * STRIDE, W * STRIDE)
    ops = HipOps('exact')
    cam = ops.depth_cam(k.to(dev), rel.to(dev).contiguous(), float(STRIDE), True)          # [2 (B + 1), 30]: forward | inverse
    cand = torch.linspace(1 / 0.5, 1 / 10.0, D, device=dev)
    rows = neighbour_rows(B, True).to(dev)
    n = B + 1

    def materialise():
        f0 = torch.stack([tok0, torch.cat([carried[1:2], tok1[:-1]], 0)], 0)
        f1 = torch.stack([tok1, torch.cat([carried[0:1], tok0[:-1]], 0)], 0)
        return f0, f1, torch.stack([cam[1:n], cam[n:2 * n - 1]], 0)

    f0, f1, cams = materialise()
    by_rows = lambda: ops.depth_corr_softmax([tok0, tok1, carried], None, H, W, cam, cand, rows=rows)
    same = torch.equal(by_rows(), ops.depth_corr_softmax(f0, f1, H, W, cams, cand))
    variants = {'rows launch': by_rows,
                'materialise + contiguous launch': lambda: ops.depth_corr_softmax(*materialise()[:2], H, W, cams, cand),
                'materialise alone': materialise,
                'contiguous launch alone': lambda: ops.depth_corr_softmax(f0, f1, H, W, cams, cand),
                'rows launch again': by_rows}
    for _ in range(2):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    lines = [f'(a) um_depth_corr_softmax_multi_rows at B={B}, {H}x{W} features, C={C}, D={D}, S=2: tok0 [{B}] | tok1 [{B}] | carried pair [2]',
             f'    {args.rounds} rounds, variants alternating, {args.iters} launches between two events; microseconds per call: median (min .. max)',
             f'    the two launches agree bit for bit on these operands: {same}', '']
    for name in variants:
        lines.append(f'    {name:34s} {fmt(times[name])}')
    spread = abs(med['rows launch again'] - med['rows launch']) / med['rows launch']
    copied = 2 * 2 * B * H * W * C * 4
    lines += ['',
              f'    rows launch / (materialise + contiguous launch): {med["rows launch"] / med["materialise + contiguous launch"]:.3f}',
              f'    rows launch / contiguous launch alone:           {med["rows launch"] / med["contiguous launch alone"]:.3f}',
              f'    rows launch against itself:                      {med["rows launch again"] / med["rows launch"]:.3f} (spread {100 * spread:.1f} %)',
              f'    materialising writes {copied / 1e6:.1f} MB (and reads as many): f0 and f1 of both sources', '']
    return lines


def sequence_part(args, dev):
    """(b): ms per depth map of the whole video."""
    frames = args.frames
    x = synth_frames(frames, 480, 640, seed=6) / 255.
    x = ((x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).contiguous().to(dev)
    k, rel = synth_camera(1, 480, 640)
    step = torch.linalg.inv(rel[0].double())
    poses = [torch.eye(4, dtype=torch.float64)]
    for _ in range(frames - 1):
        poses.append(poses[-1] @ step)
    poses = torch.stack(poses, 0).float().to(dev)
    k = k.to(dev)
    rel_next = rel.to(dev)
    pose_pair = torch.stack([rel_next[0], torch.linalg.inv(rel[0]).to(dev)], 0)[None].contiguous()
    lines = [f'(b) posed-video depth, {frames} frames 480x640 on the device (normalised already), {torch.cuda.get_device_name(0)}',
             f'    legs alternating in one process after two warm-up rounds; median of {args.reps} regions of {args.passes} passes each '
             '(min .. max); exact precision', '    ms per depth map (the sequence legs give frames - 1 maps, the per-frame loop frames - 2)', '']
    for name in ('gmdepth_s1', 'gmdepth_s1_rr1'):
        ck, fk = CONFIGS[name]
        model = UniMatch(**ck).eval()
        model.load_state_dict(synth_state_dict({key: v.shape for key, v in model.state_dict().items()}, **CONDITIONED))
        model = model.to(dev)
        kw = {key: v for key, v in fk.items() if key != 'task'}

        def seq(step, **more):
            return lambda: model.forward_sequence(x, task='depth', intrinsics=k, poses=poses, pairs_per_launch=step, **more, **kw)

        def loop():
            for t in range(1, frames - 1):
                model.forward_multiview(x[t:t + 1], torch.stack([x[t + 1], x[t - 1]], 0)[None], intrinsics=k, poses=pose_pair, **kw)

        legs = {}
        for step_ in (1, 4, 8):
            legs[f'unfused            pairs_per_launch={step_}'] = (seq(step_), frames - 1)
            legs[f'pred_bidir_depth   pairs_per_launch={step_}'] = (seq(step_, pred_bidir_depth=True), frames - 1)
            legs[f'fuse_neighbours    pairs_per_launch={step_}'] = (seq(step_, fuse_neighbours=True), frames - 1)
        legs['forward_multiview per frame (S = 2)'] = (loop, frames - 2)
        for _ in range(2):
            for fn, _maps in legs.values():
                fn()
        times = {leg: [] for leg in legs}
        for _ in range(args.reps):
            for leg, (fn, maps) in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.passes):
                    fn()
                torch.cuda.synchronize()
                times[leg].append(1e3 * (time.perf_counter() - t0) / args.passes / maps)
        lines.append(f'    {name}')
        for leg in legs:
            lines.append(f'      {leg:44s} {fmt(times[leg], digits=3)}')
        for step_ in (1, 4, 8):
            f = statistics.median(times[f'fuse_neighbours    pairs_per_launch={step_}'])
            u = statistics.median(times[f'unfused            pairs_per_launch={step_}'])
            m = statistics.median(times['forward_multiview per frame (S = 2)'])
            lines.append(f'      pairs_per_launch={step_}: fused / unfused {f / u:.3f}, fused / forward_multiview loop {f / m:.3f}')
        lines.append('')
        print('\n'.join(lines[-18:]), flush=True)
        del model
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=33)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depth_fuse_neighbours.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_depth_fuse_neighbours: no GPU (a CPU run measures nothing: not measured)')
    dev = 'cuda'
    lines = launch_part(args, dev)
    print('\n'.join(lines), flush=True)
    lines += sequence_part(args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
