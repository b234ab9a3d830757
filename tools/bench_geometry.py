"""Cost of the consistency / point-cloud kernels against a torch-op composition of the same results on the same GPU.

    python tools/bench_geometry.py [--out profiles/geometry.txt] [--frames 33] [--height 480] [--width 640]

The workload is the posed video of ``profiles/depth_sequence.txt``: 33 frames of 480 x 640.

  disparity    ``um_disp_consistency`` on 33 left / right pairs            | ``geometry.disparity_consistency_host`` on CUDA tensors
  depth        ``um_depth_consistency``, the 64 directed checks of the     | ``geometry.depth_consistency_host`` on CUDA tensors
               sequence in one launch (camera records given, masks only)   |   (the same records; it also forms the two error maps)
  points       ``um_points_pack`` of the 33 frames with a 60 % keep mask   | ``geometry.points_pack_host`` on CUDA tensors (boolean
               and colours, the read of the count and the slices included  |   indexing, which synchronises as well)

The two legs of an operation alternate inside one process after a warm-up of both; a region is as many calls as last at least 0.5 s,
timed with device events; the figure is the median of the regions, in microseconds per call.  "bytes" is what the operation must move
(inputs read once, outputs written once; the taps of the gathers are expected to hit the caches), and "HBM share" is bytes / time over
the 8 TB/s peak of an MI355X.  The file ends with the margins the GPU test holds ``um_depth_consistency`` to (4 x the largest
``|fp32 host - fp64|`` of each test case, from two host evaluations) and the kernel's own largest deviation from fp64.
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import geometry  # noqa: E402
from unimatch_amd.ops import HipOps  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 5
REGION_SECONDS = 0.5
HBM_PEAK = 8.0e12


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
    """``{name: (median, min, max) seconds per call}``; every leg warmed up, then REGIONS regions of >= REGION_SECONDS each, alternating."""
    calls = {}
    for k, fn in fns.items():
        timed(fn, 3)
        calls[k] = max(1, int(REGION_SECONDS / timed(fn, 3)) + 1)
    times = {k: [] for k in fns}
    for _ in range(REGIONS):
        for k, fn in fns.items():
            times[k].append(timed(fn, calls[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, calls


def report(lines, title, t, calls, nbytes):
    lines.append(title)
    for k, (med, lo, hi) in t.items():
        lines.append(f'  {k:<8}{med * 1e6:11.1f} us  [{lo * 1e6:.1f} .. {hi * 1e6:.1f}]   {calls[k]} calls per region')
    kernel = t['kernel'][0]
    verdict = 'the kernel is faster' if kernel < t['torch'][0] else 'THE KERNEL IS SLOWER than the torch composition'
    lines.append(f'  torch / kernel {t["torch"][0] / kernel:8.2f} x   ({verdict})')
    lines.append(f'  bytes {nbytes / 1e6:.1f} MB -> {nbytes / kernel / 1e12:.2f} TB/s, {100 * nbytes / kernel / HBM_PEAK:.0f} % of the HBM peak')
    lines.append('')
    print('\n'.join(lines[-(len(t) + 4):]), flush=True)


def scene(frames, h, w, dev):
    """A plane seen by a slowly moving camera, each depth map with 0.4 % noise: most pixels are consistent, some are not."""
    from tests import geometry_util as gu
    g = torch.Generator().manual_seed(1)
    k = gu.intrinsics_for(h, w)
    normal = torch.tensor([0.1, -0.15, 1.0], dtype=torch.float64)
    normal = normal / normal.norm()
    poses = torch.stack([gu.rigid((0.1, 1.0, 0.2), 0.01 * i, (0.04 * i, -0.01 * i, 0.01 * i)) for i in range(frames)], 0)
    depths = torch.stack([gu.plane_depth(*gu.plane_in(torch.linalg.inv(p), normal, 2.5), k, h, w) for p in poses], 0)
    depths = (depths * (1 + 0.004 * torch.randn(frames, h, w, generator=g, dtype=torch.float64))).float()
    colors = torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8)
    return depths.to(dev), k.float()[None].to(dev), poses.float().to(dev), colors.to(dev)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    from tests import geometry_util as gu
    dev = 'cuda:0'
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'geometry.txt'))
    frames, h, w = arg('--frames', 33), arg('--height', 480), arg('--width', 640)
    ops = HipOps()
    px = frames * h * w
    lines = [f'tools/bench_geometry.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'{frames} frames of {h} x {w}; per leg the median of {REGIONS} regions of >= {REGION_SECONDS} s (device events), legs alternating in one '
             'process after a warm-up of both; us per call [min .. max]', '']
    depths, k, poses, colors = scene(frames, h, w, dev)

    # disparity: the depth maps serve as smooth positive "disparities" of the right magnitude range
    dl = (depths * 8.0).contiguous()
    dr = (dl + 0.05 * torch.randn_like(dl)).contiguous()
    t, calls = alternate({'kernel': lambda: ops.disp_consistency(dl, dr), 'torch': lambda: geometry.disparity_consistency_host(dl, dr)})
    a, b = ops.disp_consistency(dl, dr), geometry.disparity_consistency_host(dl, dr)
    same = min((a[0] == b[0]).float().mean().item(), (a[1] == b[1]).float().mean().item())
    report(lines, f'disparity consistency, {frames} pairs (the two legs agree on {100 * same:.4f} % of the masks)', t, calls, px * 16)

    # depth: the 2 (T - 1) directed checks of the sequence in one launch
    n = frames - 1
    cam = ops.depth_cam(k.expand(n, 3, 3).contiguous(), ops.relative_pose_pairs(poses), 1.0, bidir=True)
    cam_inv = cam.roll(n, 0).contiguous()
    ref, src = torch.cat([depths[:-1], depths[1:]], 0), torch.cat([depths[1:], depths[:-1]], 0)
    t, calls = alternate({'kernel': lambda: ops.depth_consistency(ref, src, cam, cam_inv),
                          'torch': lambda: geometry.depth_consistency_host(ref, src, cam, cam_inv)})
    a, b = ops.depth_consistency(ref, src, cam, cam_inv), geometry.depth_consistency_host(ref, src, cam, cam_inv)[0]
    same = (a == b).float().mean().item()
    report(lines, f'depth consistency, {2 * n} directed checks in one launch, masks only ({100 * same:.4f} % equal, '
                  f'{100 * (1 - a.mean().item()):.1f} % consistent)', t, calls, 2 * n * h * w * 12)

    # points: compaction of the whole scene
    keep = (torch.rand(frames, h, w, device=dev) < 0.6).float()
    cam_world = ops.depth_cam(k.expand(frames, 3, 3).contiguous(), poses, 1.0)
    result = {}

    def kernel_leg():
        xyz, rgb, count = ops.points_pack(depths, cam_world, keep, colors, 0.0, 10.0, 1)
        m = int(count.item())
        result['kernel'] = (xyz[:m], rgb[:m])

    def torch_leg():
        result['torch'] = geometry.points_pack_host(depths, cam_world, keep, colors, 0.0, 10.0, 1)

    t, calls = alternate({'kernel': kernel_leg, 'torch': torch_leg})
    (xa, ra), (xb, rb) = result['kernel'], result['torch']
    assert xa.shape == xb.shape and torch.equal(ra, rb) and (xa - xb).abs().max().item() <= 1e-4
    share = xa.shape[0] / px
    report(lines, f'point cloud, {frames} frames, keep mask and colours, N = {xa.shape[0]} ({100 * share:.0f} % of the pixels), count read '
                  'and slices included', t, calls, px * (16 + 18 * share))

    # the margins of the GPU test and the kernel's own deviation
    lines.append('um_depth_consistency against fp64 on the cases of tests/test_geometry_gpu.py (err_px in pixels, err_rel relative)')
    lines.append('  case          margin = 4 max|fp32 host - fp64|      max|kernel - fp64|          mask pixels off (host, kernel)')
    for seed, shape in zip((101, 102, 103, 104), gu.SHAPES):
        r, s, kk, pp = gu.plane_pair(seed, *shape)
        f64, f32 = gu.depth_check_fp64(r, s, kk, pp), gu.depth_check_fp32(r, s, kk, pp)
        margin = gu.margins(f32, f64)
        got = geometry.depth_consistency_check(r.to(dev), s.to(dev), kk.to(dev), pp.to(dev), return_errors=True)
        worst = [(x.cpu().double() - y)[torch.isfinite(y)].abs().max().item() for x, y in zip(got[1:], f64[1:])]
        off = (int((f32[0].double() != f64[0]).sum()), int((got[0].cpu().double() != f64[0]).sum()))
        lines.append(f'  {str(shape):<14}{margin[0]:.2e} px  {margin[1]:.2e}            {worst[0]:.2e} px  {worst[1]:.2e}        {off}')
    text = '\n'.join(lines) + '\n'
    print('\n'.join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
