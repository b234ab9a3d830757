"""CPU tests of the TSDF fusion (unimatch_amd/fusion.py): the float32 host restatement against its float64 evaluation on the analytic
scene of tests/fusion_util.py, the surface extraction against the analytic surfaces and a direct triple loop, the semantics of
``integrate`` and of the higher-level calls, and the build wiring / C ABI without a GPU.

Measured on the three cases (float32 against float64, decided voxels): undecided share 0.04 % / 0.06 % / 0.13 %, updated share 31 % /
55 % / 70 %, no weight mismatch even inside the undecided sets, largest |tsdf32 - tsdf64| 1.3e-6 / 1.9e-6 / 2.3e-6; extraction on the
float64 volume: 537 / 1177 / 2603 points at ``min_weight = 1``, the farthest 0.37 / 0.87 / 0.67 voxel from the nearer surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, fusion, geometry, io
from tests import fusion_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [1, 2, 3]


# ------------------------------------------------------------------ 1. the float32 restatement against the float64 evaluation
@pytest.mark.parametrize('number', CASE_IDS)
def test_host_float32_against_float64(number):
    c = fu.case(number)
    t32, w32, c32 = c.host32
    t64, w64, c64 = c.host64
    assert t32.dtype == torch.float32 and t64.dtype == torch.float64 and c32.shape == (3,) + t32.shape
    print(f'case {number}: e = {c.e:.3g}, undecided {c.undecided_share:.5f}, updated {c.updated_share:.3f}, '
          f'tsdf margin {c.tsdf_margin:.3g}, weight mismatches anywhere {int((w32.double() != w64).sum())}')
    assert c.undecided_share <= 0.01                                                     # the rule leaves something to test
    if number in (1, 2):
        assert c.updated_share >= 0.25
    assert torch.equal(w32.double()[c.decided], w64[c.decided])
    err = (t32.double() - t64)[c.decided].abs().max()
    assert err <= c.tsdf_margin
    # the margin itself is what float32 allows: Xc_2 is three products and three sums of terms within M = 5 (|x| + |y| + |z| + |t| of
    # the scene), the subtraction from d one more, all divided by trunc; the running average adds at most 4 roundings of values <= 1
    # per view.  Half an ulp each: (8 M / trunc + 8 B) 2^-24 bounds the error of a decided voxel.
    assert err <= (8 * 5.0 / c.trunc + 8 * c.views) * 2.0 ** -24
    assert (c32.double() - c64)[:, c.decided].abs().max() <= 255 * 16 * c.views * 2.0 ** -24     # running means of values <= 255
    assert t64.abs().max() <= 1 and t64.min() < -0.9 and t64.max() == 1 and w64.max() <= 2 * c.views


# ------------------------------------------------------------------ 2. extraction on the float64 volume
@pytest.mark.parametrize('number', CASE_IDS)
def test_extraction_on_float64_volume(number):
    c = fu.case(number)
    t, w, col = c.plain64                                                                # weights are view counts
    for min_weight in (1.0, float(c.views)):
        xyz, rgb = fusion.extract_points_host(t, w, col, min_weight=min_weight, **c.grid)
        dist = fu.surface_distance(xyz.numpy()) / c.voxel
        print(f'case {number} min_weight {min_weight}: {xyz.shape[0]} points, farthest {dist.max():.3f} voxel')
        assert xyz.dtype == torch.float64 and rgb.dtype == torch.uint8 and rgb.shape == xyz.shape
        assert dist.max() <= 1.0
        if min_weight == 1.0:
            assert xyz.shape[0] >= 400
        want_xyz, want_rgb, where = fu.points_loop(t, w, col, fu.ORIGIN, c.voxel, min_weight)
        assert where == sorted(where) and len(where) == xyz.shape[0] > 0                 # ascending (k, j, i, axis)
        assert np.array_equal(xyz.numpy(), want_xyz) and np.array_equal(rgb.numpy(), want_rgb)
        assert torch.equal(fusion.crossings_host(t, w, min_weight).nonzero(), torch.tensor(where))
        n = xyz.shape[0]
        for capacity in (n - 1, 7, 0, n + 5):
            part, part_rgb, count = fusion.extract_points_host(t, w, col, min_weight=min_weight, capacity=capacity, **c.grid)
            assert count == n and part.shape[0] == min(n, capacity) and torch.equal(part, xyz[:capacity]) and torch.equal(part_rgb, rgb[:capacity])
    plain, none = fusion.extract_points_host(t, w, None, **c.grid)
    assert none is None and torch.equal(plain, fusion.extract_points_host(t, w, col, **c.grid)[0])


# ------------------------------------------------------------------ 3. semantics of integrate
def _volume(c, **kw):
    return fusion.TSDFVolume(fu.ORIGIN, c.voxel, c.dims, device='cpu', **kw)


def test_max_weight_clamps():
    c = fu.case(1)
    vol = _volume(c, max_weight=3., with_color=False)
    assert vol.trunc == float(np.float32(4 * np.float32(c.voxel))) and vol.color is None
    for n in range(1, 6):
        vol.integrate(c.depth, c.k, c.poses, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
        assert vol.weight.max() == min(n, 3) and set(vol.weight.unique().tolist()) == {0.0, float(min(n, 3))}
    once = _volume(c, with_color=False).integrate(c.depth, c.k, c.poses, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    seen = once.weight > 0
    # the running mean of one value repeated: five updates of three roundings each (product, sum, quotient) of values within 1
    assert torch.equal(vol.weight > 0, seen) and (vol.tsdf - once.tsdf).abs().max() <= 15 * 2.0 ** -24
    vol.reset()
    assert not vol.tsdf.any() and not vol.weight.any()


def test_pixels_without_weight_or_depth_contribute_nothing():
    c = fu.case(2)
    ref = _volume(c).integrate(c.depth, c.k, c.poses, weight=c.weight_in, colors=c.colors, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    assert torch.equal(ref.tsdf, c.host32[0]) and torch.equal(ref.weight, c.host32[1]) and torch.equal(ref.color, c.host32[2])
    dead = c.weight_in == 0
    assert 0.1 < dead.float().mean() < 0.4
    # the depth of a dead pixel does not matter, whatever it holds ...
    for bad in (float('nan'), float('inf'), 0.0, -1.5, 1e30):
        depth = torch.where(dead, torch.full_like(c.depth, bad), c.depth)
        got = _volume(c).integrate(depth, c.k, c.poses, weight=c.weight_in, colors=c.colors, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
        assert torch.equal(got.tsdf, ref.tsdf) and torch.equal(got.weight, ref.weight) and torch.equal(got.color, ref.color), bad
        # ... and a pixel with such a depth is dead without any weight: NaN, infinite, zero and negative depths contribute nothing
        weight = torch.where(dead, torch.ones_like(c.weight_in), c.weight_in)
        got = _volume(c).integrate(depth, c.k, c.poses, weight=weight, colors=c.colors, min_depth=0., max_depth=fu.MAX_DEPTH)
        assert torch.equal(got.tsdf, ref.tsdf) and torch.equal(got.weight, ref.weight) and torch.equal(got.color, ref.color), bad
    for bad in (float('nan'), float('inf'), -2.0):                                       # and so do such weights
        weight = torch.where(dead, torch.full_like(c.weight_in, bad), c.weight_in)
        got = _volume(c).integrate(c.depth, c.k, c.poses, weight=weight, colors=c.colors, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
        assert torch.equal(got.tsdf, ref.tsdf) and torch.equal(got.weight, ref.weight), bad
    assert torch.isfinite(ref.tsdf).all() and torch.isfinite(ref.color).all()


def test_camera_looking_away_contributes_nothing():
    c = fu.case(1)
    flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0]))                              # half a turn about y: the volume is behind
    vol = _volume(c).integrate(c.depth, c.k, c.poses @ flip, colors=c.colors, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    assert not vol.tsdf.any() and not vol.weight.any() and not vol.color.any()
    with pytest.raises(ValueError, match='colors'):
        vol.integrate(c.depth, c.k, c.poses)
    with pytest.raises(ValueError, match='colors'):
        _volume(c, with_color=False).integrate(c.depth, c.k, c.poses, colors=c.colors)
    with pytest.raises(ValueError, match='weight'):
        vol.integrate(c.depth, c.k, c.poses, weight=c.weight_in[:, :-1], colors=c.colors)
    for bad in (dict(voxel_size=0.), dict(voxel_size=float('nan')), dict(trunc=-1.), dict(max_weight=0.), dict(dims=(4, 0, 4)),
                dict(dims=(2048, 2048, 512))):
        with pytest.raises(ValueError):
            fusion.TSDFVolume(**dict(dict(origin=fu.ORIGIN, voxel_size=0.05, dims=(4, 4, 4), device='cpu'), **bad))


# ------------------------------------------------------------------ 4. the higher-level calls
def test_fuse_depth_sequence_tsdf_chunking_and_refusal():
    c = fu.case(3)
    kw = dict(colors=c.colors, weight=c.weight_in, voxel_size=0.05, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    outs = [fusion.fuse_depth_sequence_tsdf(c.depth, c.k, c.poses, views_per_launch=n, **kw) for n in (1, 2, c.views)]
    first = outs[0]
    vol = first['volume']
    assert first['xyz'].shape[0] >= 400 and first['rgb'].shape == first['xyz'].shape
    assert (fu.surface_distance(first['xyz'].double().numpy()) / 0.05).max() <= 1.0
    for other in outs[1:]:
        assert torch.equal(other['xyz'], first['xyz']) and torch.equal(other['rgb'], first['rgb'])
        for name in ('tsdf', 'weight', 'color'):
            assert torch.equal(getattr(other['volume'], name), getattr(vol, name)), name
    # the box: the kept points, padded by the truncation distance
    lo, hi = fusion.volume_bounds(c.depth, c.k, c.poses, keep=(c.weight_in > 0).float(), min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    pts, _ = geometry.back_project_points(c.depth, c.k, c.poses, keep=(c.weight_in > 0).float(), stride=4)
    assert np.allclose(lo, pts.amin(0).numpy()) and np.allclose(hi, pts.amax(0).numpy())
    assert np.allclose(vol.origin, np.asarray(lo) - vol.trunc, atol=1e-6) and vol.trunc == float(np.float32(4 * np.float32(0.05)))
    top = np.asarray(vol.origin) + (np.asarray(vol.dims) - 1) * vol.voxel_size
    assert (top >= np.asarray(hi) + vol.trunc - 1e-5).all() and (top < np.asarray(hi) + vol.trunc + vol.voxel_size).all()
    plain = fusion.fuse_depth_sequence_tsdf(c.depth, c.k, c.poses, voxel_size=0.05, max_depth=fu.MAX_DEPTH)
    assert plain['rgb'] is None and plain['volume'].color is None and plain['xyz'].shape[0] > first['xyz'].shape[0]
    with pytest.raises(ValueError, match=r'max_voxels=5000; use voxel_size >= 0\.\d+') as exc:
        fusion.fuse_depth_sequence_tsdf(c.depth, c.k, c.poses, max_voxels=5000, **kw)
    named = float(re.search(r'voxel_size >= ([0-9.]+)', str(exc.value)).group(1))
    assert named > 0.05
    coarse = fusion.fuse_depth_sequence_tsdf(c.depth, c.k, c.poses, max_voxels=5000, **dict(kw, voxel_size=named * 1.001))   # the named size fits
    assert int(np.prod(coarse['volume'].dims)) <= 5000                                # (the padding alone is 9 voxels per axis)
    with pytest.raises(ValueError, match='no pixel'):
        fusion.volume_bounds(c.depth, c.k, c.poses, keep=torch.zeros_like(c.depth))


class DepthStandIn:
    """Both entry points of the depth runner: the analytic depth of each frame, in order."""

    def __init__(self, depths):
        self.depths, self.next = depths, 0

    def predict(self, ref, tgt, inference_size=None, **kw):
        i, self.next = self.next, self.next + 1
        return {'flow_preds': [self.depths[i:i + 1]]}

    def forward_sequence(self, frames, carry=None, **kw):
        first = 0 if carry is None else carry['index']
        n = frames.shape[0] - (1 if carry is None else 0)
        assert tuple(frames.shape[-2:]) == tuple(self.depths.shape[-2:])
        return {'depth': self.depths[first:first + n], 'carry': {'index': first + n}}


@pytest.mark.parametrize('mode', ['default', 'sequence'])
def test_runner_writes_the_tsdf_surface(tmp_path, mode):
    pytest.importorskip('PIL')
    from unimatch_amd import depth
    views, h, w = 5, 24, 40
    k, poses = fu.cameras(views, h, w, 7)
    depths = fu.render(k, poses, h, w).float()
    rng = np.random.default_rng(11)
    scene = tmp_path / 'scene'
    for sub in ('color', 'pose', 'intrinsic'):
        os.makedirs(scene / sub)
    for i in range(views):
        io.write_png8(str(scene / 'color' / f'{i:04d}.png'), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        np.savetxt(str(scene / 'pose' / f'{i:04d}.txt'), poses[i].double().numpy())
    k4 = np.eye(4)
    k4[:3, :3] = k[0].double().numpy()
    np.savetxt(str(scene / 'intrinsic' / 'intrinsic_depth.txt'), k4)
    imgs, poses_read, k_read = depth.read_scene(str(scene))
    common = dict(padding_factor=8, device='cpu', pairs_per_launch=2 if mode == 'sequence' else None, rel_thr=0.05, px_thr=2.0)
    ply = str(tmp_path / 'surface.ply')
    n = depth.run_depth(DepthStandIn(depths), str(scene), str(tmp_path / 'out'), {}, save_tsdf_ply=ply, voxel_size=0.05,
                        tsdf_min_weight=1.0, **common)
    assert n == views - 1 and sorted(os.listdir(tmp_path / 'out')) == [f'{i:04d}.png' for i in range(views - 1)]     # no other file
    xyz, rgb = io.read_ply(ply)
    assert xyz.shape[0] >= 400 and rgb.shape == xyz.shape and rgb.dtype == np.uint8
    assert (fu.surface_distance(xyz.astype(np.float64)) / 0.05).max() <= 1.0
    # exactly the pixels --save-ply keeps, as the integration weight
    from unimatch_amd.video import read_frame_u8
    t = views - 1
    kk, pp = torch.from_numpy(k_read)[None], torch.from_numpy(poses_read[:t])
    colors = torch.stack([read_frame_u8(f) for f in imgs[:t]], 0)
    cloud = geometry.fuse_depth_sequence(depths[:t], kk, pp, colors, px_thr=2.0, rel_thr=0.05)
    assert 0.5 < cloud['keep'].mean() < 1.0
    want = fusion.fuse_depth_sequence_tsdf(depths[:t], kk, pp, colors, weight=cloud['keep'], voxel_size=0.05)
    assert np.array_equal(xyz, want['xyz'].numpy()) and np.array_equal(rgb, want['rgb'].numpy())
    assert xyz.shape[0] < cloud['xyz'].shape[0]                                          # one surface, not one point per pixel and frame
    # together with --save-ply, and the parser
    both = str(tmp_path / 'cloud.ply')
    depth.run_depth(DepthStandIn(depths), str(scene), str(tmp_path / 'out2'), {}, save_ply=both, save_tsdf_ply=ply, voxel_size=0.05, **common)
    assert np.array_equal(io.read_ply(both)[0], cloud['xyz'].numpy()) and np.array_equal(io.read_ply(ply)[0], xyz)
    with pytest.raises(SystemExit):
        depth.main(['--scene', 'x', '--out', 'y', '--save-tsdf-ply', 'f.ply', '--voxel-size', 'small'])


# ------------------------------------------------------------------ 5. build wiring and the C ABI without a GPU
def test_build_wiring():
    from unimatch_amd.build import EXTRA_FLAGS, RESOURCE_GUARDS, SOURCES
    assert 'fusion.hip' in SOURCES and EXTRA_FLAGS['fusion.hip'] == EXTRA_FLAGS['geometry.hip']
    assert '-ffp-contract=off' in EXTRA_FLAGS['fusion.hip']
    source = open(os.path.join(ROOT, 'unimatch_amd', 'csrc', 'fusion.hip')).read()
    kernels = set(re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', source))
    assert kernels == set(RESOURCE_GUARDS['fusion.hip']) and len(kernels) == 4
    assert set(RESOURCE_GUARDS['fusion.hip'].values()) == set(RESOURCE_GUARDS['geometry.hip'].values()) == {4}
    assert 'atomic' not in source.split('#include')[1:][-1].lower()                      # no atomics below the header comment


def test_fusion_symbols_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(os.path.join(ROOT, 'include', 'unimatch_hip.h')).read()
    fp = ctypes.POINTER(ctypes.c_float)
    v, i, z, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    want = {'um_tsdf_integrate': (i, [v] * 7 + [i] * 3 + [fp] + [f] * 5 + [i] * 3 + [v]),
            'um_tsdf_points_workspace_bytes': (z, [i] * 3),
            'um_tsdf_points': (i, [v] * 3 + [i] * 3 + [fp] + [f] * 2 + [v] * 3 + [i, v, z, v])}
    for name, sig in want.items():
        assert f'{name}(' in text and hasattr(lib, name) and _abi.SIGNATURES[name] == sig, name
        decl = re.search(r'\n(?:int|size_t) ' + name + r'\(([^;]*)\);', text).group(1)
        assert len(decl.split(',')) == len(sig[1]), name                 # the declaration has as many parameters as the binding
    assert int(re.search(r'#define UM_VERSION (\d+)', text).group(1)) == 220 == _abi.load().um_version()
    assert len(_abi.CENSUS) == 15


def test_fusion_abi_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(4096)
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, big = float('nan'), 1 << 11

    def err():
        return lib.um_last_error_string()

    assert lib.um_tsdf_points_workspace_bytes(37, 29, 23) == -(-37 * 29 * 23 // 256) * 2 * 4
    assert lib.um_tsdf_points_workspace_bytes(2048, 1024, 1023) > 0
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1), (2048, 1024, 1024), (65536, 65536, 1)):
        assert lib.um_tsdf_points_workspace_bytes(*bad) == 0, bad
    good = dict(depth=p, cam=p, weight_in=None, colors=p, tsdf=p, weight=p, color=p, nx=8, ny=8, nz=8, origin=origin, voxel=0.05, trunc=0.2,
                max_weight=64.0, min_depth=0.0, max_depth=10.0, batch=1, h=8, w=8, stream=None)
    cases = [dict(depth=None), dict(cam=None), dict(tsdf=None), dict(weight=None), dict(origin=None), dict(colors=None), dict(color=None),
             dict(nx=0), dict(ny=-1), dict(nz=0), dict(batch=0), dict(h=0), dict(w=0), dict(nx=big, ny=big, nz=512), dict(batch=big, h=big, w=512),
             dict(voxel=0.0), dict(voxel=nan), dict(trunc=-0.1), dict(trunc=nan), dict(max_weight=0.0), dict(max_weight=nan)]
    for change in cases:
        lib.um_tsdf_points_workspace_bytes(0, 0, 0)
        lib.um_image_warp(None, 0, p, p, None, 1, 3, 8, 8, 0, None)                      # another entry point's message in between
        assert lib.um_tsdf_integrate(*dict(good, **change).values()) == -1 and b'um_tsdf_integrate' in err(), change
    good = dict(tsdf=p, weight=p, color=p, nx=8, ny=8, nz=8, origin=origin, voxel=0.05, min_weight=1.0, xyz=p, rgb=p, count=p, capacity=16,
                ws=p, ws_bytes=1 << 20, stream=None)
    cases = [dict(tsdf=None), dict(weight=None), dict(origin=None), dict(xyz=None), dict(count=None), dict(color=None), dict(rgb=None),
             dict(nx=0), dict(ny=0), dict(nz=-3), dict(nx=big, ny=big, nz=512), dict(capacity=-1), dict(voxel=0.0), dict(voxel=nan),
             dict(min_weight=nan)]
    for change in cases:
        lib.um_image_warp(None, 0, p, p, None, 1, 3, 8, 8, 0, None)
        assert lib.um_tsdf_points(*dict(good, **change).values()) == -1 and b'um_tsdf_points' in err(), change
    for change in (dict(ws=None), dict(ws_bytes=15), dict(ws=ctypes.c_void_p(4098))):    # 8 x 8 x 8: two workgroups, 16 bytes
        assert lib.um_tsdf_points(*dict(good, **change).values()) == -3 and b'um_tsdf_points' in err(), change
    assert lib.um_tsdf_points_workspace_bytes(8, 8, 8) == 16
