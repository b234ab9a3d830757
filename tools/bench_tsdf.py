"""Cost of the TSDF fusion kernels on a posed video: against a torch-op composition, one launch against B, against a plain copy.

    python tools/bench_tsdf.py [--out profiles/tsdf.txt] [--frames 33] [--height 480] [--width 640] [--voxels 0.02,0.01]

The workload: the analytic scene of tests/fusion_util.py (a plane behind a sphere) seen by 33 cameras of 480 x 640, each depth map with
0.3 % noise, colours, and a 70 % keep mask as the integration weight; the volume is the box (-1.6, -1.2, 0.9) .. (1.6, 1.2, 2.5) at each
voxel size.  Per voxel size, four measurements:

  (a) integrate    ``um_tsdf_integrate``, all views in one launch   | ``fusion.integrate_host`` on CUDA tensors: the restatement's
                                                                    |   torch composition (the convention of tools/bench_geometry.py)
  (b) views        one B-view launch                                | B one-view launches of the same kernel
  (c) copy         the B-view launch's bytes per second             | ``um_probe_copy`` of as many bytes, measured in the same run
  (d) extract      ``TSDFVolume.extract_points``: three launches, the read of the count and the slices

"bytes" of the B-view launch: every plane of the volume read once and written once (tsdf, weight, three colour planes: 40 bytes per
voxel; voxels no view reaches are not written, so this is an upper bound) plus the depth, weight and colour maps once (11 bytes per
pixel).  B one-view launches move the volume B times.

Every measurement runs in a child process of its own under its own time limit (``--limit`` seconds, default 240); a measurement that
fails or runs out of time is recorded as such and nothing further is started.  The legs of a measurement alternate inside one process
after a warm-up of each; a region is as many calls as last at least 0.3 s, timed with device events; the figure is the median of 5
regions, in microseconds per call.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARGV = sys.argv[1:]
REGIONS = 5
REGION_SECONDS = 0.3
HBM_PEAK = 8.0e12
BOX = ((-1.6, -1.2, 0.9), (1.6, 1.2, 2.5))
PARTS = ('integrate', 'views', 'extract')


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def timed(fn, calls):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / calls


def alternate(fns):
    """``{name: [median, min, max, calls per region]}`` in seconds per call; every leg warmed up, then REGIONS regions, alternating."""
    calls = {}
    for k, fn in fns.items():
        timed(fn, 2)
        calls[k] = max(1, int(REGION_SECONDS / timed(fn, 2)) + 1)
    times = {k: [] for k in fns}
    for _ in range(REGIONS):
        for k, fn in fns.items():
            times[k].append(timed(fn, calls[k]))
    return {k: [statistics.median(v), min(v), max(v), calls[k]] for k, v in times.items()}


def scene(frames, h, w, dev):
    import torch
    from tests import fusion_util as fu
    k, poses = fu.cameras(frames, h, w, 1)
    g = torch.Generator().manual_seed(2)
    depth = fu.render(k, poses, h, w)
    depth = (depth * (1 + 0.003 * torch.randn(frames, h, w, generator=g, dtype=torch.float64))).float()
    colors = torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8)
    weight = (torch.rand(frames, h, w, generator=g) < 0.7).float()
    return depth.to(dev), k.to(dev), poses.to(dev), weight.to(dev), colors.to(dev)


def measure(part, voxel, frames, h, w):
    """One measurement in this process: a JSON line on stdout."""
    import torch
    from unimatch_amd import _abi, fusion, geometry
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    dev = 'cuda:0'
    depth, k, poses, weight, colors = scene(frames, h, w, dev)
    dims = tuple(int(round((b - a) / voxel)) for a, b in zip(*BOX))
    vol = fusion.TSDFVolume(BOX[0], voxel, dims, device=dev)
    cam = geometry._cam_pack(k.expand(frames, 3, 3).contiguous(), poses, True)[frames:].contiguous()
    kw = dict(origin=vol.origin, voxel=vol.voxel_size, trunc=vol.trunc, max_weight=vol.max_weight, min_depth=0.1, max_depth=10.0)
    state = (vol.tsdf, vol.weight, vol.color)
    voxels = dims[0] * dims[1] * dims[2]
    out = {'part': part, 'voxel': voxel, 'dims': dims, 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}

    def fused():
        fusion.integrate_device(*state, depth, cam, weight, colors, **kw)

    if part == 'integrate':
        out['t'] = alternate({'kernel': fused, 'torch': lambda: fusion.integrate_host(*state, depth, cam, weight, colors, **kw)})
        vol.reset()
        fused()
        want = fusion.integrate_host(*(torch.zeros_like(t) for t in state), depth, cam, weight, colors, **kw)
        out['equal'] = [float((a.view(torch.int32) == b.view(torch.int32)).float().mean()) for a, b in zip(state, want)]
        out['updated'] = float((vol.weight > 0).float().mean())
    elif part == 'views':
        views = [(depth[i:i + 1].contiguous(), cam[i:i + 1].contiguous(), weight[i:i + 1].contiguous(), colors[i:i + 1].contiguous())
                 for i in range(frames)]

        def one_by_one():
            for v in views:
                fusion.integrate_device(*state, *v, **kw)

        nbytes = (voxels * 40 + frames * h * w * 11 + 15) // 16 * 16
        src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        lib = _abi.load()

        def copy():                                                                      # reads nbytes / 2, writes nbytes / 2
            _abi.check(lib.um_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes // 32 * 16, torch.cuda.current_stream().cuda_stream), 'um_probe_copy')

        out['t'] = alternate({'fused': fused, 'single': one_by_one, 'copy': copy})
        out['bytes'] = nbytes
        out['copy_bytes'] = nbytes // 32 * 16 * 2
    else:
        fused()
        result = {}

        def extract():
            result['n'] = vol.extract_points()[0].shape[0]

        out['t'] = alternate({'extract': extract})
        out['points'] = result['n']
        out['capacity'] = 6 * (dims[0] * dims[1] + dims[1] * dims[2] + dims[0] * dims[2])
    print('RESULT ' + json.dumps(out), flush=True)


def us(t):
    return f'{t[0] * 1e6:11.1f} us  [{t[1] * 1e6:.1f} .. {t[2] * 1e6:.1f}]   {t[3]} calls per region'


def main():
    frames, h, w = arg('--frames', 33), arg('--height', 480), arg('--width', 640)
    if '--part' in ARGV:
        return measure(arg('--part', ''), arg('--voxel', 0.02), frames, h, w)
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'tsdf.txt'))
    limit = arg('--limit', 240)
    lines, failed = [], None
    for voxel in [float(v) for v in arg('--voxels', '0.02,0.01').split(',')]:
        for part in PARTS:
            cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--voxel', str(voxel), '--frames', str(frames), '--height', str(h),
                   '--width', str(w)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                res = [ln for ln in done.stdout.splitlines() if ln.startswith('RESULT ')]
                if done.returncode != 0 or not res:
                    failed = f'{part} at voxel {voxel}: exit status {done.returncode}: {done.stderr.strip().splitlines()[-1:]}'
            except subprocess.TimeoutExpired:
                failed = f'{part} at voxel {voxel}: no result within its time limit of {limit} s'
            if failed:
                lines += [f'NOT MEASURED -- {failed}; nothing further was started', '']
                break
            r = json.loads(res[0][7:])
            t, dims = r['t'], r['dims']
            if not lines:
                lines += [f'tools/bench_tsdf.py on {r["device"]}, torch {r["torch"]}',
                          f'{frames} views of {h} x {w}; per leg the median of {REGIONS} regions of >= {REGION_SECONDS} s (device events), legs alternating '
                          f'in one process after a warm-up of each; us per call [min .. max]; every measurement in its own process, limit {limit} s', '']
            head = f'voxel {voxel} m, volume {dims[0]} x {dims[1]} x {dims[2]} = {dims[0] * dims[1] * dims[2] / 1e6:.2f} M voxels'
            if part == 'integrate':
                verdict = 'the kernel is faster' if t['kernel'][0] < t['torch'][0] else 'THE KERNEL IS SLOWER than the torch composition'
                lines += [f'(a) {head}: um_tsdf_integrate, {frames} views in one launch, against the torch composition on the GPU',
                          f'  kernel  {us(t["kernel"])}', f'  torch   {us(t["torch"])}',
                          f'  torch / kernel {t["torch"][0] / t["kernel"][0]:8.2f} x   ({verdict})',
                          f'  {100 * r["updated"]:.1f} % of the voxels updated; bitwise equal to the composition on '
                          f'{" / ".join(f"{100 * e:.4f} %" for e in r["equal"])} of tsdf / weight / color', '']
            elif part == 'views':
                rate, copy_rate = r['bytes'] / t['fused'][0], r['copy_bytes'] / t['copy'][0]
                lines += [f'(b) {head}: one {frames}-view launch against {frames} one-view launches',
                          f'  fused   {us(t["fused"])}', f'  single  {us(t["single"])}',
                          f'  single / fused {t["single"][0] / t["fused"][0]:8.2f} x',
                          f'(c) the fused launch moves {r["bytes"] / 1e6:.1f} MB (volume read + written once, maps read once): {rate / 1e12:.2f} TB/s, '
                          f'{100 * rate / HBM_PEAK:.0f} % of the HBM peak',
                          f'  copy    {us(t["copy"])}   um_probe_copy of {r["copy_bytes"] / 1e6:.1f} MB (read + written): {copy_rate / 1e12:.2f} TB/s',
                          f'  fused / copy bytes per second {rate / copy_rate:8.2f}', '']
            else:
                lines += [f'(d) {head}: extract_points, N = {r["points"]} points (first capacity {r["capacity"]} rows), count read and slices included',
                          f'  extract {us(t["extract"])}', '']
            print('\n'.join(lines[-8:]), flush=True)
        if failed:
            break
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if failed:
        raise SystemExit(failed)


if __name__ == '__main__':
    main()
