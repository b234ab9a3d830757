"""Cost of the TSDF mesh extraction (um_tsdf_mesh) on the fused volume of a posed video: against the torch composition of its host
restatement, against the surface points of the same volume, against a plain copy of as many bytes.

    python tools/bench_tsdf_mesh.py [--out profiles/tsdf_mesh.txt] [--frames 33] [--height 480] [--width 640] [--voxels 0.02,0.01]

The workload is that of tools/bench_tsdf.py: its analytic scene seen by 33 cameras of 480 x 640 with noise, colours and a 70 % keep mask,
fused by ``um_tsdf_integrate`` into the box (-1.6, -1.2, 0.9) .. (1.6, 1.2, 2.5) at each voxel size.  Per voxel size, one measurement of
four alternating legs on that volume:

  mesh     ``fusion.mesh_device`` at the default capacities of ``TSDFVolume.extract_mesh``: the five launches of ``um_tsdf_mesh``, no
           read of the counts
  torch    ``fusion.extract_mesh_host`` on the same CUDA tensors: the baseline (the convention of tools/bench_geometry.py)
  points   ``fusion.points_device`` on the same volume: the floor, one count and one scatter traversal of the same planes
  copy     ``um_probe_copy`` of as many bytes as the mesh passes must move

"bytes" of the mesh: per voxel, tsdf and weight read once (8), the cell code written and read twice (2 + 2 + 2), the vertex mask
written and read once (1 + 1), the vertex base written (4) -- 20 bytes; per vertex its row (15 with colour) and the two ends of its edge
in four planes (32); per face its row (12) and the bases and masks of its cell's seven edge owners (35).  The neighbour taps of the
cell and classify passes are counted once: they overlap between adjacent lanes and rows, so this is the compulsory traffic.

Every measurement runs in a child process of its own under its own time limit (``--limit`` seconds, default 300); one that fails or
runs out of time is recorded as such and nothing further is started.  Legs alternate inside the process after a warm-up of each; a
region is as many calls as last at least 0.3 s, timed with device events; the figure is the median of 5 regions, in microseconds per
call.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_tsdf as base                                       # noqa: E402  (the scene, the timing loop and the formatting)

ARGV = sys.argv[1:]


def measure(voxel, frames, h, w, trace=False):
    """One measurement in this process: a JSON line on stdout."""
    import torch
    from unimatch_amd import _abi, fusion, geometry
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    dev = 'cuda:0'
    depth, k, poses, weight, colors = base.scene(frames, h, w, dev)
    dims = tuple(int(round((b - a) / voxel)) for a, b in zip(*base.BOX))
    vol = fusion.TSDFVolume(base.BOX[0], voxel, dims, device=dev)
    cam = geometry._cam_pack(k.expand(frames, 3, 3).contiguous(), poses, True)[frames:].contiguous()
    fusion.integrate_device(vol.tsdf, vol.weight, vol.color, depth, cam, weight, colors, origin=vol.origin, voxel=vol.voxel_size,
                            trunc=vol.trunc, max_weight=vol.max_weight, min_depth=0.1, max_depth=10.0)
    del depth, weight, colors
    state, grid = (vol.tsdf, vol.weight, vol.color), dict(origin=vol.origin, voxel=vol.voxel_size)
    vcap, fcap = vol._mesh_capacities()
    pcap = 6 * (dims[0] * dims[1] + dims[1] * dims[2] + dims[0] * dims[2])
    xyz, rgb = torch.empty((vcap, 3), device=dev), torch.empty((vcap, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((fcap, 3), dtype=torch.int32, device=dev)

    def mesh():
        return fusion.mesh_device(*state, vertex_capacity=vcap, face_capacity=fcap, xyz=xyz, rgb=rgb, faces=faces, **grid)

    pts_xyz, pts_rgb = torch.empty((pcap, 3), device=dev), torch.empty((pcap, 3), dtype=torch.uint8, device=dev)

    def points():
        return fusion.points_device(*state, capacity=pcap, xyz=pts_xyz, rgb=pts_rgb, **grid)

    v, f = (int(n) for n in mesh()[3].tolist())
    n_points = int(points()[2].item())
    if trace:                                                                            # under rocprofv3: a few calls of each, no timing
        for _ in range(20):
            mesh()
            points()
        torch.cuda.synchronize()
        return
    voxels = dims[0] * dims[1] * dims[2]
    nbytes = (voxels * 20 + v * (15 + 32) + f * (12 + 35) + 31) // 32 * 32
    src = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
    lib = _abi.load()

    def copy():                                                                          # reads nbytes / 2, writes nbytes / 2
        _abi.check(lib.um_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes // 2, torch.cuda.current_stream().cuda_stream), 'um_probe_copy')

    out = {'voxel': voxel, 'dims': dims, 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'V': v, 'F': f,
           'points': n_points, 'capacities': [vcap, fcap], 'bytes': nbytes, 'workspace': int(lib.um_tsdf_mesh_workspace_bytes(*dims))}
    out['t'] = base.alternate({'mesh': mesh, 'torch': lambda: fusion.extract_mesh_host(*state, **grid), 'points': points, 'copy': copy})
    want = fusion.extract_mesh_host(*state, **grid)
    out['equal'] = [float((xyz[:v].view(torch.int32) == want[0].view(torch.int32)).float().mean()), float((rgb[:v] == want[1]).float().mean()),
                    float((faces[:f].long() == want[2]).float().mean())]
    print('RESULT ' + json.dumps(out), flush=True)


def kernel_trace(voxel, frames, h, w, limit):
    """Per-kernel times of the last voxel size from ``rocprofv3 --kernel-trace --stats``, in a run of its own (21 calls of each entry
    point): the lines for the report."""
    import csv
    import glob
    import shutil
    import tempfile
    tool = shutil.which('rocprofv3')
    if not tool:
        return ['kernel times: NOT MEASURED -- rocprofv3 is not on the path', '']
    out_dir = tempfile.mkdtemp(prefix='tsdf_mesh_trace_')
    cmd = [tool, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 't', '--', sys.executable,
           os.path.abspath(__file__), '--one', '--trace-child', '--voxel', str(voxel), '--frames', str(frames), '--height', str(h), '--width', str(w)]
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=out_dir, env=dict(os.environ, TMPDIR='/tmp'))
    except subprocess.TimeoutExpired:
        return [f'kernel times: NOT MEASURED -- no trace within {limit} s', '']
    stats = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if done.returncode != 0 or not stats:
        return [f'kernel times: NOT MEASURED -- rocprofv3 exit status {done.returncode}, {len(stats)} stats files', '']
    rows = [r for r in csv.DictReader(open(stats[0])) if 'tsdf_mesh' in r.get('Name', '') or 'tsdf_points' in r.get('Name', '')]
    shutil.rmtree(out_dir, ignore_errors=True)
    lines = [f'kernel times at voxel {voxel} m (rocprofv3 --kernel-trace --stats, a run of its own, tracing on): calls, average us']
    lines += [f'  {r["Name"].split("(")[0]:34s} {r.get("Calls", "?"):>5s} {float(r.get("AverageNs", "nan")) / 1e3:10.1f}' for r in rows]
    return lines + ['']


def main():
    frames, h, w = base.arg('--frames', 33), base.arg('--height', 480), base.arg('--width', 640)
    if '--one' in ARGV:
        return measure(base.arg('--voxel', 0.02), frames, h, w, trace='--trace-child' in ARGV)
    out_path = base.arg('--out', os.path.join(ROOT, 'profiles', 'tsdf_mesh.txt'))
    limit = base.arg('--limit', 300)
    lines, failed = [], None
    for voxel in [float(v) for v in base.arg('--voxels', '0.02,0.01').split(',')]:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '--voxel', str(voxel), '--frames', str(frames), '--height', str(h),
               '--width', str(w)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            res = [ln for ln in done.stdout.splitlines() if ln.startswith('RESULT ')]
            if done.returncode != 0 or not res:
                failed = f'voxel {voxel}: exit status {done.returncode}: {done.stderr.strip().splitlines()[-1:]}'
        except subprocess.TimeoutExpired:
            failed = f'voxel {voxel}: no result within its time limit of {limit} s'
        if failed:
            lines += [f'NOT MEASURED -- {failed}; nothing further was started', '']
            break
        r = json.loads(res[0][7:])
        t, dims = r['t'], r['dims']
        voxels = dims[0] * dims[1] * dims[2]
        if not lines:
            lines += [f'tools/bench_tsdf_mesh.py on {r["device"]}, torch {r["torch"]}',
                      f'{frames} views of {h} x {w} fused first; per leg the median of {base.REGIONS} regions of >= {base.REGION_SECONDS} s '
                      f'(device events), legs alternating in one process after a warm-up of each; us per call [min .. max]; every voxel '
                      f'size in its own process, limit {limit} s', '']
        rate, copy_rate = r['bytes'] / t['mesh'][0], r['bytes'] / t['copy'][0]
        verdict = 'the kernel is faster' if t['mesh'][0] < t['torch'][0] else 'THE KERNEL IS SLOWER than the torch composition'
        lines += [f'voxel {voxel} m, volume {dims[0]} x {dims[1]} x {dims[2]} = {voxels / 1e6:.2f} M voxels: V = {r["V"]} vertices, F = {r["F"]} faces '
                  f'(capacities {r["capacities"][0]} / {r["capacities"][1]} rows), {r["points"]} surface points; workspace '
                  f'{r["workspace"] / 1e6:.1f} MB',
                  f'  mesh    {base.us(t["mesh"])}   um_tsdf_mesh, five launches',
                  f'  torch   {base.us(t["torch"])}   extract_mesh_host on the GPU',
                  f'  points  {base.us(t["points"])}   um_tsdf_points, three launches',
                  f'  copy    {base.us(t["copy"])}   um_probe_copy of {r["bytes"] / 1e6:.1f} MB (read + written)',
                  f'  torch / mesh {t["torch"][0] / t["mesh"][0]:8.2f} x   ({verdict})',
                  f'  mesh / points {t["mesh"][0] / t["points"][0]:7.2f} x',
                  f'  the mesh passes move at least {r["bytes"] / 1e6:.1f} MB = {r["bytes"] / voxels:.1f} bytes per voxel: {rate / 1e12:.2f} TB/s, '
                  f'{100 * rate / base.HBM_PEAK:.0f} % of the HBM peak; the copy probe moves them at {copy_rate / 1e12:.2f} TB/s: mesh / copy time '
                  f'{t["mesh"][0] / t["copy"][0]:.2f} x',
                  f'  bitwise equal to the composition on {" / ".join(f"{100 * e:.4f} %" for e in r["equal"])} of xyz / rgb / faces', '']
        print('\n'.join(lines[-11:]), flush=True)
    if not failed and '--kernel-trace' in ARGV:
        lines += kernel_trace(voxel, frames, h, w, limit)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if failed:
        raise SystemExit(failed)


if __name__ == '__main__':
    main()
