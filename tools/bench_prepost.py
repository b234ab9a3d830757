"""Cost of the inference-size handling around the model: the torch-op pipeline the package used before against the
``InferenceGeometry`` pipeline (um_image_prepare / um_pred_restore).

    python tools/bench_prepost.py [--out profiles/prepost.txt] [--iters 20] [--frames 9]

Two cases, each at batch 1 and batch 8, the model itself left out (a fixed prediction at the inference size stands in for it):

  flow    1080 x 1920 -> 768 x 1344: two images in, one flow back
    torch     fp32 NCHW frames, ``F.interpolate`` in, ``F.interpolate`` out and the two in-place slice rescales (video.run_directory)
    geometry  uint8 NHWC frames, ``InferenceGeometry.resized``: ``prepare`` and ``restore``
  stereo  375 x 1242 padded to a multiple of 32: two images in (ImageNet-normalised), one disparity back
    torch     fp32 NCHW frames, ``(x / 255 - mean) / std`` with torch ops on the device (the loaders do it on the host, which costs
              more), ``InputPadder.pad``, ``unpad(...).contiguous()`` (a tensor of its own, which is what ``restore`` returns)
    geometry  uint8 NHWC frames, ``InferenceGeometry.padded``: ``prepare(normalize=True)`` and ``restore``

Each case is timed twice: ``device`` with the frames already on the device (the kernels and their launches alone), ``upload`` from
pageable host tensors (12 bytes per pixel against 3).  Every figure is the median of 7 synchronised regions of ``--iters`` calls
(synchronize, wall clock, synchronize) after a warm-up of every leg, the legs alternating inside one process; the spread is (max -
min) / median over the regions.  ``GB/s`` is the traffic the geometry pipeline needs (source + destination bytes of its three
launches) over its device time, against the 8.0 TB/s HBM peak of the MI355X: at these sizes launches and host work dominate.

Then ``video.run_directory`` end to end over ``--frames`` synthetic 1080 x 1920 PNG frames (gmflow_s1, seeded weights, inference size
768 x 1344), with and without ``device_resize``: ms per pair, median of 3 runs each, alternating.
"""
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import UniMatch, video  # noqa: E402
from unimatch_amd.io import InputPadder, write_png8  # noqa: E402
from unimatch_amd.prepost import IMAGENET_MEAN, IMAGENET_STD, InferenceGeometry  # noqa: E402
from unimatch_amd.synth import CONFIGS, synth_state_dict  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 7
HBM_PEAK = 8.0e12


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


def frames(b, h, w, seed):
    u = torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u, u.permute(0, 3, 1, 2).float().contiguous()


def flow_case(b):
    (h, w), size = (1080, 1920), (768, 1344)
    (u0, f0), (u1, f1) = frames(b, h, w, 1), frames(b, h, w, 2)
    pred = torch.randn(b, 2, *size, device='cuda')
    geom = InferenceGeometry.resized((h, w), size)

    def torch_ops(a, c):
        a = F.interpolate(a, size=size, mode='bilinear', align_corners=True)
        c = F.interpolate(c, size=size, mode='bilinear', align_corners=True)
        flow = F.interpolate(pred, size=(h, w), mode='bilinear', align_corners=True)
        flow[:, 0] = flow[:, 0] * w / size[-1]
        flow[:, 1] = flow[:, 1] * h / size[-2]
        return a, c, flow

    def geometry(a, c):
        a, c = geom.prepare(a, c)
        return a, c, geom.restore(pred, 'flow')

    traffic = 2 * b * (3 * h * w + 12 * size[0] * size[1]) + b * 8 * (size[0] * size[1] + h * w)
    return f'flow {h} x {w} -> {size[0]} x {size[1]}', (f0, f1), (u0, u1), torch_ops, geometry, traffic


def stereo_case(b):
    h, w = 375, 1242
    (u0, f0), (u1, f1) = frames(b, h, w, 3), frames(b, h, w, 4)
    padder = InputPadder((b, 3, h, w), padding_factor=32)
    geom = InferenceGeometry.padded((h, w), 'sintel', 32)
    hp, wp = geom.size
    pred = torch.rand(b, hp, wp, device='cuda') * 190
    mean, std = (torch.tensor(c, device='cuda').view(1, 3, 1, 1) for c in (IMAGENET_MEAN, IMAGENET_STD))

    def torch_ops(a, c):
        a, c = padder.pad((a / 255 - mean) / std, (c / 255 - mean) / std)
        return a, c, padder.unpad(pred).contiguous()

    def geometry(a, c):
        a, c = geom.prepare(a, c, normalize=True)
        return a, c, geom.restore(pred, 'disparity')

    traffic = 2 * b * (3 * h * w + 12 * hp * wp) + b * 4 * (hp * wp + h * w)
    return f'stereo {h} x {w} padded to {hp} x {wp}', (f0, f1), (u0, u1), torch_ops, geometry, traffic


def pipeline_rows(make, b, iters, lines):
    title, host_f, host_u, torch_ops, geometry, traffic = make(b)
    dev_f, dev_u = [x.cuda() for x in host_f], [x.cuda() for x in host_u]
    legs = {'torch    device': lambda: torch_ops(*dev_f), 'geometry device': lambda: geometry(*dev_u),
            'torch    upload': lambda: torch_ops(*(x.cuda() for x in host_f)),
            'geometry upload': lambda: geometry(*(x.cuda() for x in host_u))}
    t = alternate(legs, iters)
    lines.append(f'{title}, batch {b}: two images in, one prediction back (ms per call: median, spread over {REGIONS} regions of {iters} calls)')
    for k, (med, spread) in t.items():
        lines.append(f'  {k:<18}{1e3 * med:9.4f}   spread {100 * spread:5.1f} %')
    for kind in ('device', 'upload'):
        tt, tg = t[f'torch    {kind}'], t[f'geometry {kind}']
        allow = max(tt[1], tg[1])
        verdict = 'not slower' if tg[0] <= tt[0] * (1 + allow) else 'SLOWER'
        lines.append(f'  {kind}: torch / geometry {tt[0] / tg[0]:6.2f} x   -> geometry is {verdict} (allowance: the spread, {100 * allow:.1f} %)')
    rate = traffic / t['geometry device'][0]
    lines.append(f'  geometry traffic {traffic / 1e6:.1f} MB -> {rate / 1e9:.0f} GB/s = {100 * rate / HBM_PEAK:.1f} % of the HBM peak')
    lines.append('')
    print('\n'.join(lines[-9:]), flush=True)


def directory_rows(count, lines):
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}))
    model = model.cuda()
    kw = {k: v for k, v in fk.items() if k != 'task'}
    tmp = tempfile.mkdtemp(prefix='bench_prepost_')
    try:
        rng = np.random.default_rng(0)
        base = rng.integers(0, 256, (1080 // 8 + 2, 1920 // 8 + 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
        os.makedirs(os.path.join(tmp, 'in'))
        for i in range(count):                           # a blocky texture that moves two pixels per frame
            write_png8(os.path.join(tmp, 'in', f'{i:04d}.png'), np.ascontiguousarray(base[4:1084, 2 * i:2 * i + 1920]))
        paths = video.list_frames(os.path.join(tmp, 'in'))
        times = {'torch ops': [], 'device_resize': []}

        def run(flag):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = video.run_directory(model, paths, os.path.join(tmp, 'out'), kw, inference_size=(768, 1344), pairs_per_launch=4,
                                    device_resize=flag)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        run(False), run(True)
        for _ in range(3):
            times['torch ops'].append(run(False))
            times['device_resize'].append(run(True))
        lines.append(f'video.run_directory, gmflow_s1 exact, {count} PNG frames 1080 x 1920 -> 768 x 1344, 4 pairs per launch, files written '
                     '(ms per pair: median, spread over 3 runs)')
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        for k in times:
            lines.append(f'  {k:<18}{1e3 * med[k]:9.2f}   spread {100 * spread[k]:5.1f} %')
        allow = max(spread.values())
        verdict = 'not slower' if med['device_resize'] <= med['torch ops'] * (1 + allow) else 'SLOWER'
        lines.append(f'  torch ops / device_resize {med["torch ops"] / med["device_resize"]:6.3f} x   -> device_resize is {verdict} '
                     f'(allowance: the spread, {100 * allow:.1f} %)')
        lines.append('')
        print('\n'.join(lines[-5:]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'prepost.txt'))
    iters, count = arg('--iters', 20), arg('--frames', 9)
    lines = [f'tools/bench_prepost.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'median of {REGIONS} synchronised regions of {iters} calls per leg, legs alternating in one process, every leg warmed up once',
             'torch = the torch-op pipeline (fp32 frames); geometry = InferenceGeometry on um_image_prepare / um_pred_restore (uint8 frames)', '']
    for make in (flow_case, stereo_case):
        for b in (1, 8):
            pipeline_rows(make, b, iters, lines)
    directory_rows(count, lines)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
