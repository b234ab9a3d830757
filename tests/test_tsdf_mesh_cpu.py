"""CPU tests of the TSDF mesh extraction (``fusion.extract_mesh_host``, the restatement of ``um_tsdf_mesh``): against the direct triple
loop of tests/tsdf_mesh_util.py on an analytic sphere and on the fused scene of tests/fusion_util.py, the topology the definition
promises (watertight, consistently oriented, outward normals), the validity rule, the PLY mesh files, the runner, and the build wiring /
C ABI without a GPU.

The sphere of the issue (37 x 29 x 23, radius 8.4 voxels): 3966 vertices, 7928 faces, 11892 edges."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, fusion, io
from tests import fusion_util as fu
from tests import tsdf_mesh_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


def vertex_bound(ref, voxel):
    """What float32 allows a vertex coordinate after its float32 voxel centre: the subtraction, the quotient, the product and the sum,
    half an ulp each, with the margin of tests/test_fusion_gpu.py."""
    return 8 * EPS32 * (np.abs(ref) + float(np.float32(voxel)))


# ------------------------------------------------------------------ 1. the analytic closed surface
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['float32', 'float64'])
def test_sphere_against_the_loop_and_its_topology(dtype):
    t, w, col = (v.to(dtype) for v in mu.sphere())
    grid = dict(origin=mu.SPHERE_ORIGIN, voxel=mu.SPHERE_VOXEL)
    xyz, rgb, faces = fusion.extract_mesh_host(t, w, col, **grid)
    assert xyz.dtype == dtype and rgb.dtype == torch.uint8 and rgb.shape == xyz.shape and faces.shape[1] == 3
    assert (xyz.shape[0], faces.shape[0]) == (3966, 7928)
    assert not (t == 0).any()                                                            # no corner lies on the surface
    want_xyz, want_rgb, want_faces, where, _ = mu.mesh_loop(t, w, col, mu.SPHERE_ORIGIN, mu.SPHERE_VOXEL, 1.0,
                                                           centre=np.float32 if dtype == torch.float32 else np.float64)
    assert np.array_equal(faces.numpy(), want_faces)
    err = np.abs(xyz.double().numpy() - want_xyz)
    print(f'{dtype}: largest |xyz - loop| {err.max():.3g}, largest share of the bound {(err / vertex_bound(want_xyz, mu.SPHERE_VOXEL)).max():.3f}')
    if dtype == torch.float64:
        assert np.array_equal(xyz.numpy(), want_xyz) and np.array_equal(rgb.numpy(), want_rgb)
    else:
        assert (err <= vertex_bound(want_xyz, mu.SPHERE_VOXEL)).all()
        assert np.abs(rgb.numpy().astype(int) - want_rgb.astype(int)).max() <= 1           # a colour next to a rounding boundary
    mu.assert_closed_outward(xyz.numpy(), faces.numpy(), mu.SPHERE_CENTRE)
    # vertices ascend strictly in (k, j, i, e): the selection of the restatement is the loop's, row for row
    _, sel = fusion.mesh_edges_host(t, w)
    k, j, i, a = sel.nonzero(as_tuple=True)
    assert list(zip(k.tolist(), j.tolist(), i.tolist(), (a + 1).tolist())) == where
    assert all(x < y for x, y in zip(where, where[1:]))
    plain, none, same = fusion.extract_mesh_host(t, w, None, **grid)
    assert none is None and torch.equal(plain, xyz) and torch.equal(same, faces)


# ------------------------------------------------------------------ 2. the fused scene: a surface with a boundary
@pytest.mark.parametrize('which', ['host32', 'plain64'])
def test_fused_scene(which):
    c = fu.case(3)
    t, w, col = getattr(c, which)
    min_weight = 2.0 if which == 'host32' else float(c.views)
    xyz, rgb, faces = fusion.extract_mesh_host(t, w, col, min_weight=min_weight, **c.grid)
    per_edge, repeats, _ = mu.topology(faces.numpy())
    print(f'{which}: V = {xyz.shape[0]}, F = {faces.shape[0]}, faces per edge {per_edge}')
    assert faces.shape[0] > 1000 and per_edge == {1, 2} and repeats == 1                 # a boundary, and still manifold and oriented
    assert len(np.unique(faces.numpy())) == xyz.shape[0]
    # the vertices on axis edges are points of extract_points_host, bit for bit and in the same relative order ...
    active, sel = fusion.mesh_edges_host(t, w, min_weight)
    axis = sel[..., [0, 1, 3]]                                                           # e = 1, 2, 4
    cross = fusion.crossings_host(t, w, min_weight)
    assert not (axis & ~cross).any() and axis.sum() > 500
    pts, pts_rgb = fusion.extract_points_host(t, w, col, min_weight=min_weight, **c.grid)
    e = sel.nonzero(as_tuple=True)[3] + 1
    mine = (e == 1) | (e == 2) | (e == 4)
    theirs = axis[cross]                                                                 # per point, in its order: is it a mesh vertex
    assert torch.equal(xyz[mine], pts[theirs]) and torch.equal(rgb[mine], pts_rgb[theirs])
    # ... and every crossing that lies in an active cell is among them (the cells of an axis edge, from the validity rule alone)
    valid = ((w >= min_weight) & (t.abs() < 1)).numpy()
    nz, ny, nx = valid.shape
    cell = np.zeros((nz + 1, ny + 1, nx + 1), bool)                                      # cell (i, j, k) at [k + 1, j + 1, i + 1]
    cell[1:nz, 1:ny, 1:nx] = np.all([valid[m >> 2 & 1:nz - 1 + (m >> 2 & 1), m >> 1 & 1:ny - 1 + (m >> 1 & 1), (m & 1):nx - 1 + (m & 1)]
                                     for m in range(8)], 0)
    assert np.array_equal(cell[1:nz, 1:ny, 1:nx], active.numpy())
    for a, others in enumerate(((1, 2), (0, 2), (0, 1))):
        near = np.zeros((nz, ny, nx), bool)
        for s in range(4):
            d = [0, 0, 0]
            d[others[0]], d[others[1]] = s & 1, s >> 1
            near |= cell[1 - d[2]:nz + 1 - d[2], 1 - d[1]:ny + 1 - d[1], 1 - d[0]:nx + 1 - d[0]]
        assert np.array_equal(axis[..., a].numpy(), cross[..., a].numpy() & near), a


# ------------------------------------------------------------------ 3. the validity rule
def _keyed(tsdf, weight, min_weight=1.0):
    """The loop's mesh with every face as its three edges ``(k, j, i, e)`` and its cell."""
    xyz, _, faces, where, cells = mu.mesh_loop(tsdf, weight, None, (0.5, -1.0, 2.0), 0.25, min_weight)
    return xyz, [tuple(where[v] for v in f) for f in faces.tolist()], where, cells


@pytest.mark.parametrize('how', ['weight', 'value', 'nan'])
def test_one_invalid_corner_removes_the_faces_of_its_cells(how):
    nx, ny, nz = 5, 4, 3
    g = torch.Generator().manual_seed(17)
    sign = torch.where(torch.rand(nz, ny, nx, generator=g) < 0.5, -1.0, 1.0)
    base = (sign * (0.05 + 0.9 * torch.rand(nz, ny, nx, generator=g))).double()
    weight = torch.full((nz, ny, nx), 2.0, dtype=torch.float64)
    grid = dict(origin=(0.5, -1.0, 2.0), voxel=0.25)
    xyz0, keyed0, where0, cells0 = _keyed(base, weight)
    assert len(keyed0) > 50
    for p in ((2, 1, 1), (0, 0, 0), (4, 3, 2), (3, 0, 1)):                               # interior, two corners of the box, a side
        t, w = base.clone(), weight.clone()
        if how == 'weight':
            w[p[2], p[1], p[0]] = 0.5
        else:
            t[p[2], p[1], p[0]] = {'value': float(torch.sign(base[p[2], p[1], p[0]])), 'nan': float('nan')}[how]
        around = {(p[2] - dk, p[1] - dj, p[0] - di) for dk in (0, 1) for dj in (0, 1) for di in (0, 1)}
        expect = [f for f, cell in zip(keyed0, cells0) if cell not in around]
        assert len(expect) < len(keyed0)
        xyz1, keyed1, where1, _ = _keyed(t, w)
        assert keyed1 == expect                                                          # exactly the faces of its up to eight cells go
        assert where1 == sorted({v for f in expect for v in f})                          # and the vertices nothing references any more
        assert np.array_equal(xyz1, xyz0[[where0.index(v) for v in where1]])             # the others keep their place
        got_xyz, _, got_faces = fusion.extract_mesh_host(t, w, None, **grid)
        assert np.array_equal(got_xyz.numpy(), xyz1)
        assert [tuple(where1[v] for v in f) for f in got_faces.tolist()] == expect


def test_volumes_without_a_cell_give_an_empty_mesh():
    for shape in ((1, 4, 5), (4, 1, 5), (4, 5, 1), (1, 1, 1)):
        t = torch.linspace(-0.9, 0.9, int(np.prod(shape))).reshape(shape)
        xyz, rgb, faces = fusion.extract_mesh_host(t, torch.ones(shape), torch.zeros((3,) + shape), origin=(0, 0, 0), voxel=0.1)
        assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and rgb.dtype == torch.uint8 and faces.shape == (0, 3)
        assert mu.mesh_loop(t, torch.ones(shape), None, (0, 0, 0), 0.1, 1.0)[2].shape == (0, 3)
    # a volume with cells and no valid voxel, and one entirely on one side
    t = torch.full((3, 4, 5), 0.5)
    for w in (torch.zeros(3, 4, 5), torch.ones(3, 4, 5)):
        xyz, none, faces = fusion.extract_mesh_host(t, w, None, origin=(0, 0, 0), voxel=0.1)
        assert xyz.shape == (0, 3) and none is None and faces.shape == (0, 3)
    vol = fusion.TSDFVolume((0, 0, 0), 0.1, (5, 4, 3), device='cpu')
    assert [tuple(v.shape) for v in vol.extract_mesh()] == [(0, 3)] * 3


# ------------------------------------------------------------------ 4. the C ABI without a GPU
def test_mesh_symbols_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(os.path.join(ROOT, 'include', 'unimatch_hip.h')).read()
    fp = ctypes.POINTER(ctypes.c_float)
    v, i, z, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    want = {'um_tsdf_mesh_workspace_bytes': (z, [i] * 3),
            'um_tsdf_mesh': (i, [v] * 3 + [i] * 3 + [fp] + [f] * 2 + [v] * 4 + [i, i, v, z, v])}
    for name, sig in want.items():
        assert f'{name}(' in text and hasattr(lib, name) and _abi.SIGNATURES[name] == sig, name
        decl = re.search(r'\n(?:int|size_t) ' + name + r'\(([^;]*)\);', text).group(1)
        assert len(decl.split(',')) == len(sig[1]), name                 # the declaration has as many parameters as the binding
    assert int(re.search(r'#define UM_VERSION (\d+)', text).group(1)) == 220 == _abi.load().um_version()
    assert len(_abi.CENSUS) == 15


def test_mesh_abi_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(4096)
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, big = float('nan'), 1 << 11

    def err():
        return lib.um_last_error_string()

    groups = -(-37 * 29 * 23 // 256)
    assert lib.um_tsdf_mesh_workspace_bytes(37, 29, 23) == groups * 16 + 37 * 29 * 23 * 7
    assert lib.um_tsdf_mesh_workspace_bytes(2048, 1024, 1023) > 7 * 2048 * 1024 * 1023
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1), (2048, 1024, 1024), (65536, 65536, 1)):
        assert lib.um_tsdf_mesh_workspace_bytes(*bad) == 0, bad
    good = dict(tsdf=p, weight=p, color=p, nx=8, ny=8, nz=8, origin=origin, voxel=0.05, min_weight=1.0, xyz=p, rgb=p, faces=p, counts=p,
                vertex_capacity=16, face_capacity=16, ws=p, ws_bytes=1 << 20, stream=None)
    cases = [dict(tsdf=None), dict(weight=None), dict(origin=None), dict(xyz=None), dict(faces=None), dict(counts=None), dict(color=None),
             dict(rgb=None), dict(nx=0), dict(ny=0), dict(nz=-3), dict(nx=big, ny=big, nz=512), dict(vertex_capacity=-1),
             dict(face_capacity=-1), dict(voxel=0.0), dict(voxel=nan), dict(min_weight=nan)]
    for change in cases:
        lib.um_image_warp(None, 0, p, p, None, 1, 3, 8, 8, 0, None)                      # another entry point's message in between
        assert lib.um_tsdf_mesh(*dict(good, **change).values()) == -1 and b'um_tsdf_mesh' in err(), change
    need = 2 * 16 + 512 * 7                                                              # 8 x 8 x 8: two workgroups
    assert lib.um_tsdf_mesh_workspace_bytes(8, 8, 8) == need
    for change in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(4098))):
        assert lib.um_tsdf_mesh(*dict(good, **change).values()) == -3 and b'um_tsdf_mesh' in err(), change


# ------------------------------------------------------------------ 5. build wiring
def test_mesh_build_wiring():
    from unimatch_amd.build import EXTRA_FLAGS, HEADERS, RESOURCE_GUARDS, SOURCES
    assert 'tsdf_mesh.hip' in SOURCES and EXTRA_FLAGS['tsdf_mesh.hip'] == EXTRA_FLAGS['fusion.hip']
    source = open(os.path.join(ROOT, 'unimatch_amd', 'csrc', 'tsdf_mesh.hip')).read()
    kernels = set(re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', source))
    assert kernels == set(RESOURCE_GUARDS['tsdf_mesh.hip']) and len(kernels) == 5
    assert set(RESOURCE_GUARDS['tsdf_mesh.hip'].values()) == {4}
    assert 'atomic' not in source.split('#include')[1:][-1].lower()                      # no atomics below the header comment
    for included in re.findall(r'#include "(\w+\.h)"', source):
        assert included in HEADERS, included                                             # a change of a header rebuilds the source
    fused = open(os.path.join(ROOT, 'unimatch_amd', 'csrc', 'fusion.hip')).read()
    assert set(re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', fused)) == set(RESOURCE_GUARDS['fusion.hip'])
    assert len(RESOURCE_GUARDS['fusion.hip']) == 4


# ------------------------------------------------------------------ 6. files and the runner
def test_ply_mesh_round_trip(tmp_path):
    t, w, col = (v.float() for v in mu.sphere())
    xyz, rgb, faces = fusion.extract_mesh_host(t, w, col, origin=mu.SPHERE_ORIGIN, voxel=mu.SPHERE_VOXEL)
    name = str(tmp_path / 'mesh.ply')
    for colours in (rgb.numpy(), None):
        for f in (faces.numpy(), faces.numpy().astype(np.int32)):
            io.write_ply_mesh(name, xyz.numpy(), colours, f)
            got = io.read_ply_mesh(name)
            assert np.array_equal(got[0], xyz.numpy()) and np.array_equal(got[2], faces.numpy()) and got[2].dtype == np.int32
            assert (got[1] is None) if colours is None else np.array_equal(got[1], rgb.numpy())
    size = os.path.getsize(name)
    head = open(name, 'rb').read().split(b'end_header\n')[0].decode('ascii')
    assert 'element face 7928\nproperty list uchar int vertex_indices\n' in head and head.startswith('ply\nformat binary_little_endian 1.0\n')
    assert size == len(head) + len('end_header\n') + 3966 * 12 + 7928 * 13
    cloud = str(tmp_path / 'cloud.ply')
    io.write_ply(cloud, xyz.numpy(), None)
    assert open(name, 'rb').read().split(b'end_header\n', 1)[1][:3966 * 12] == open(cloud, 'rb').read().split(b'end_header\n', 1)[1]
    with pytest.raises(ValueError):
        io.read_ply(name)                                                                # the point reader still refuses a mesh
    with pytest.raises(ValueError):
        io.read_ply_mesh(cloud)
    io.write_ply_mesh(name, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    got = io.read_ply_mesh(name)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[2].dtype == np.int32
    bad = faces.numpy().copy()
    for value, shape in ((-1, None), (3966, None), (0, (-1, 4)), (0, (-1,))):
        f = bad.copy()
        f[5, 1] = value
        with pytest.raises(ValueError):
            io.write_ply_mesh(name, xyz.numpy(), rgb.numpy(), f if shape is None else f.reshape(shape))
    with pytest.raises(ValueError):
        io.write_ply_mesh(name, xyz.numpy(), rgb.numpy(), bad.astype(np.float32))


@pytest.mark.parametrize('mode', ['default', 'sequence'])
def test_runner_writes_the_tsdf_mesh(tmp_path, mode):
    pytest.importorskip('PIL')
    from unimatch_amd import depth, geometry
    from unimatch_amd.video import read_frame_u8
    from tests.test_fusion_cpu import DepthStandIn
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
    mesh = str(tmp_path / 'mesh.ply')
    n = depth.run_depth(DepthStandIn(depths), str(scene), str(tmp_path / 'out'), {}, save_tsdf_mesh=mesh, voxel_size=0.05,
                        tsdf_min_weight=1.0, **common)
    assert n == views - 1 and sorted(os.listdir(tmp_path / 'out')) == [f'{i:04d}.png' for i in range(views - 1)]     # no other file
    xyz, rgb, faces = io.read_ply_mesh(mesh)
    t = views - 1
    kk, pp = torch.from_numpy(k_read)[None], torch.from_numpy(poses_read[:t])
    colors = torch.stack([read_frame_u8(f) for f in imgs[:t]], 0)
    cloud = geometry.fuse_depth_sequence(depths[:t], kk, pp, colors, px_thr=2.0, rel_thr=0.05)
    want = fusion.fuse_depth_sequence_tsdf(depths[:t], kk, pp, colors, weight=cloud['keep'], voxel_size=0.05, mesh=True)
    assert sorted(want) == ['faces', 'rgb', 'volume', 'xyz'] and want['faces'].shape[0] > 500
    assert np.array_equal(xyz, want['xyz'].numpy()) and np.array_equal(rgb, want['rgb'].numpy())
    assert np.array_equal(faces, want['faces'].numpy())
    assert (fu.surface_distance(xyz.astype(np.float64)) / 0.05).max() <= 1.0
    per_edge, repeats, _ = mu.topology(faces)
    assert per_edge <= {1, 2} and repeats == 1
    # without mesh=True nothing changes, and with both options one volume gives both files
    points = fusion.fuse_depth_sequence_tsdf(depths[:t], kk, pp, colors, weight=cloud['keep'], voxel_size=0.05)
    assert sorted(points) == ['rgb', 'volume', 'xyz'] and torch.equal(points['volume'].tsdf, want['volume'].tsdf)
    ply = str(tmp_path / 'surface.ply')
    depth.run_depth(DepthStandIn(depths), str(scene), str(tmp_path / 'out2'), {}, save_tsdf_ply=ply, save_tsdf_mesh=mesh, voxel_size=0.05,
                    **common)
    assert np.array_equal(io.read_ply(ply)[0], points['xyz'].numpy()) and np.array_equal(io.read_ply(ply)[1], points['rgb'].numpy())
    assert np.array_equal(io.read_ply_mesh(mesh)[2], faces) and np.array_equal(io.read_ply_mesh(mesh)[0], xyz)
    # a scene with no kept pixel: an empty mesh
    depth.run_depth(DepthStandIn(depths), str(scene), str(tmp_path / 'out3'), {}, save_tsdf_mesh=mesh, voxel_size=0.05,
                    **dict(common, rel_thr=0.0, px_thr=0.0))
    assert [v.shape for v in io.read_ply_mesh(mesh)] == [(0, 3)] * 3
    with pytest.raises(SystemExit):
        depth.main(['--scene', 'x', '--out', 'y', '--save-tsdf-mesh'])
