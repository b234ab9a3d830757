"""Posed-video depth: the runner's pairwise ``predict`` loop against its sequence mode (``run_depth(pairs_per_launch=N)``).

    python tools/bench_depth_sequence.py [--out profiles/depth_sequence.txt] [--frames 33] [--reps 5] [--passes 8]

Scene: synthetic, ``--frames`` frames of 480 x 640 (``synth.synth_frames`` as uint8, ``synth_camera``'s relative pose accumulated into
absolute poses), held in memory: ``depth.read_scene`` / ``read_frame_u8`` are replaced by look-ups and ``io.write_png8`` by a no-op, so
both legs are the runner's own code (``unimatch_amd.depth.run_depth``) without the image codec -- uploads, pose arithmetic, prepare,
model, restore, colouring and the copies back are all inside the timed region.  Models ``gmdepth_s1`` and ``gmdepth_s1_rr1``
(conditioned synthetic weights, exact precision).  Legs: ``pairs_per_launch=None`` (one ``predict`` per pair, the default mode) and
1, 4, 8.  Every leg is warmed up twice, then the legs alternate; a region is ``--passes`` runs of the scene between two device
synchronisations; the median of ``--reps`` regions is reported with the spread (min .. max).  In separate, untimed passes: the images
the CNN encoder sees, and the synchronising torch calls (``torch.cuda.set_sync_debug_mode('warn')`` warnings: device-to-host copies,
``.item()``, ...) per frame.
"""
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import UniMatch, depth, io  # noqa: E402
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_frames, synth_state_dict  # noqa: E402

ARGV = sys.argv[1:]
H, W = 480, 640
LEGS = (None, 1, 4, 8)


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def memory_scene(frames):
    """Puts a synthetic scene behind the runner's readers; returns the number of frames."""
    names = [f'{i:04d}.png' for i in range(frames)]
    images = dict(zip(names, synth_frames(frames, H, W, seed=6).permute(0, 2, 3, 1).round().to(torch.uint8).contiguous()))
    k, rel = synth_camera(1, H, W)
    step = np.linalg.inv(rel[0].double().numpy())
    poses = [np.eye(4)]
    for _ in range(frames - 1):
        poses.append(poses[-1] @ step)
    poses = np.stack(poses, 0).astype(np.float32)
    depth.read_scene = lambda scene_dir: (names, poses, k[0].numpy())
    depth.read_frame_u8 = images.__getitem__
    io.write_png8 = lambda path, image: None
    return frames


def model_for(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    return model.cuda(), fk


def region(fn, passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / passes


def counts(model, fn):
    """(images the encoder saw, synchronising torch calls) of one untimed run of ``fn``."""
    seen = [0]
    inner = model.backbone.forward

    def counted(x, *a, **k):
        seen[0] += x.shape[0] if torch.is_tensor(x) else sum(t.shape[0] for t in x)
        return inner(x, *a, **k)
    model.backbone.forward = counted
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
        del model.backbone.forward
    return seen[0], sum('synchroniz' in str(w.message).lower() for w in caught)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_depth_sequence: no GPU (a CPU run measures nothing: not measured)')
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'depth_sequence.txt'))
    frames, reps, passes = memory_scene(arg('--frames', 33)), arg('--reps', 5), arg('--passes', 8)
    lines = [f'posed-video depth, {frames} frames {H}x{W} (synthetic scene in memory, no image codec), {torch.cuda.get_device_name(0)}',
             f'runner legs alternated in one process; median of {reps} regions of {passes} scene passes each (min .. max); exact precision',
             'pairs_per_launch None = the pairwise predict loop of the default mode', '']
    for name in ('gmdepth_s1', 'gmdepth_s1_rr1'):
        model, fk = model_for(name)
        legs = {n: (lambda n=n: depth.run_depth(model, 'memory', os.path.join(ROOT, 'profiles'), fk, pairs_per_launch=n)) for n in LEGS}
        for _ in range(2):                                # warm-up: code objects, caches, allocator, every chunk shape of the scene
            for fn in legs.values():
                fn()
        times = {n: [] for n in LEGS}
        for _ in range(reps):
            for n, fn in legs.items():
                times[n].append(region(fn, passes))
        base = statistics.median(times[None])
        lines.append(f'{name}')
        lines.append(f'  {"pairs_per_launch":>16} {"ms/frame":>9} {"min":>7} {"max":>7} {"vs pairwise":>11} {"encoder images":>14} {"syncs/frame":>11}')
        for n in LEGS:
            med = statistics.median(times[n])
            images, syncs = counts(model, legs[n])
            lines.append(f'  {str(n):>16} {1e3 * med / frames:9.3f} {1e3 * min(times[n]) / frames:7.3f} {1e3 * max(times[n]) / frames:7.3f} '
                         f'{base / med:10.2f}x {images:14d} {syncs / frames:11.2f}')
        lines.append('')
        print('\n'.join(lines[-(len(LEGS) + 3):]), flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines))


if __name__ == '__main__':
    main()
