"""GPU tests of the TSDF mesh extraction: ``um_tsdf_mesh`` (csrc/tsdf_mesh.hip) BITWISE against the float32 host restatement
``fusion.extract_mesh_host`` and against the float64 triple loop of tests/tsdf_mesh_util.py.

The volumes are the analytic sphere (37 x 29 x 23) and the device-integrated cases of tests/fusion_util.py (nx = 37, 40, 48: ragged
against 64-wide waves; 24679 to 69120 voxels: many 256-thread workgroups with a ragged last one).  One larger sphere volume
(96 x 64 x 48 = 1152 workgroups, so every thread of the single scan workgroup walks a run of two counts) covers the long scan; the host
and loop results are computed once per volume and shared.

Measured, float32 restatement against the float64 loop after the float32 voxel centre (the bound is 8 * 2^-24 * (|ref| + voxel) per
coordinate): the largest share of the bound any coordinate uses is 0.12 on the sphere and 0.11 / 0.14 / 0.16 on cases 1 / 2 / 3 (on the
host-integrated volumes, which equal the device-integrated ones bit for bit), diagonal edges included -- the bound of
tests/test_fusion_gpu.py is not widened."""
import functools

import numpy as np
import pytest
import torch

from unimatch_amd import fusion, geometry
from tests import fusion_util as fu
from tests import memory_guard as mg
from tests import tsdf_mesh_util as mu
from tests.test_fusion_gpu import device_result

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VOLUMES = ['sphere', 1, 2, 3]


@functools.lru_cache(maxsize=None)
def volume(name):
    """``(tsdf, weight, color, grid, min_weight)`` on the host in float32: the sphere, or a case as ``um_tsdf_integrate`` left it."""
    if name == 'sphere':
        return tuple(v.float() for v in mu.sphere()) + (dict(origin=mu.SPHERE_ORIGIN, voxel=mu.SPHERE_VOXEL), 1.0)
    return tuple(device_result(name)) + (fu.case(name).grid, 0.5)


@functools.lru_cache(maxsize=None)
def host_mesh(name, color=True):
    t, w, col, grid, min_weight = volume(name)
    return fusion.extract_mesh_host(t, w, col if color else None, min_weight=min_weight, **grid)


@functools.lru_cache(maxsize=None)
def device_mesh(name, color=True):
    t, w, col, grid, min_weight = volume(name)
    vol = on_device(t, w, col if color else None, grid)
    return tuple(None if v is None else v.cpu() for v in vol.extract_mesh(min_weight))


def on_device(t, w, col, grid):
    nz, ny, nx = t.shape
    vol = fusion.TSDFVolume(grid['origin'], grid['voxel'], (nx, ny, nz), with_color=col is not None, device=DEV)
    vol.tsdf.copy_(t)
    vol.weight.copy_(w)
    if col is not None:
        vol.color.copy_(col)
    return vol


def assert_mesh_equal(got, want):
    xyz, rgb, faces = (None if v is None else v.cpu() for v in got)
    assert xyz.shape == want[0].shape and faces.shape == want[2].shape, (xyz.shape, want[0].shape, faces.shape, want[2].shape)
    same = xyz.view(torch.int32) == want[0].view(torch.int32)
    assert bool(same.all()), f'xyz: {int((~same).sum())} of {same.numel()} values differ, the largest by {float((xyz - want[0]).abs().max())}'
    assert (rgb is None and want[1] is None) or torch.equal(rgb, want[1])
    assert faces.dtype == torch.int32 and torch.equal(faces.long(), want[2])


# ------------------------------------------------------------------ 1. bitwise against the float32 restatement
@pytest.mark.parametrize('color', [True, False], ids=['colour', 'plain'])
@pytest.mark.parametrize('name', VOLUMES)
def test_device_bitwise_against_host(name, color):
    want = host_mesh(name, color)
    assert want[0].shape[0] > 500 and want[2].shape[0] > 800
    assert_mesh_equal(device_mesh(name, color), want)


# ------------------------------------------------------------------ 2. against the float64 loop
@pytest.mark.parametrize('name', VOLUMES)
def test_device_against_float64_loop(name):
    t, w, col, grid, min_weight = volume(name)
    xyz, rgb, faces = device_mesh(name)
    ref, ref_rgb, ref_faces, where, _ = mu.mesh_loop(t, w, col, grid['origin'], grid['voxel'], min_weight, centre=np.float32)
    assert np.array_equal(faces.numpy(), ref_faces)
    bound = 8 * 2.0 ** -24 * (np.abs(ref) + float(np.float32(grid['voxel'])))
    err = np.abs(xyz.double().numpy() - ref)
    diagonal = np.array([e not in (1, 2, 4) for *_, e in where])
    print(f'{name}: V = {len(ref)}, F = {len(ref_faces)}, largest share of the bound: axis edges {(err / bound)[~diagonal].max():.3f}, '
          f'diagonal edges {(err / bound)[diagonal].max():.3f}')
    assert diagonal.sum() > len(where) // 3 and (err <= bound).all()
    assert np.abs(rgb.numpy().astype(int) - ref_rgb.astype(int)).max() <= 1              # a colour next to a rounding boundary


# ------------------------------------------------------------------ 3. topology of the device result
def test_device_sphere_topology():
    xyz, _, faces = device_mesh('sphere')
    assert (xyz.shape[0], faces.shape[0]) == (3966, 7928)
    mu.assert_closed_outward(xyz.numpy(), faces.numpy(), mu.SPHERE_CENTRE)


# ------------------------------------------------------------------ 4. capacities
def test_capacities_and_the_second_run(monkeypatch):
    t, w, col, grid, min_weight = volume(2)
    want = host_mesh(2)
    v, f = want[0].shape[0], want[2].shape[0]
    dev = [x.to(DEV) for x in (t, w, col)]
    for vcap, fcap in ((v - 1, f - 1), (7, f + 3), (v + 3, 5), (v, f)):
        xyz = torch.full((v + 4, 3), -777.0, device=DEV)
        rgb = torch.full((v + 4, 3), 93, dtype=torch.uint8, device=DEV)
        faces = torch.full((f + 4, 3), -5, dtype=torch.int32, device=DEV)
        *_, counts = fusion.mesh_device(*dev, min_weight=min_weight, vertex_capacity=vcap, face_capacity=fcap, xyz=xyz[:vcap], rgb=rgb[:vcap],
                                        faces=faces[:fcap], **grid)
        assert counts.tolist() == [v, f], (vcap, fcap)                                   # the full counts, whatever the capacities
        nv, nf = min(v, vcap), min(f, fcap)
        assert torch.equal(xyz[:nv].cpu(), want[0][:nv]) and torch.equal(rgb[:nv].cpu(), want[1][:nv])
        assert torch.equal(faces[:nf].cpu().long(), want[2][:nf])                        # true indices, also those past vertex_capacity
        assert bool((xyz[nv:] == -777.0).all()) and bool((rgb[nv:] == 93).all()) and bool((faces[nf:] == -5).all())
    assert int(want[2].max()) == v - 1 > 7                                               # (7, f + 3) wrote indices past its vertex rows
    vol = on_device(t, w, col, grid)
    calls = []
    real = fusion.mesh_device

    def counting(*args, **kw):
        calls.append((kw['vertex_capacity'], kw['face_capacity']))
        return real(*args, **kw)

    monkeypatch.setattr(fusion, 'mesh_device', counting)
    assert_mesh_equal(vol.extract_mesh(min_weight), want)
    assert len(calls) == 1 and calls[0][0] >= v and calls[0][1] >= f                     # the defaults hold this surface: one run
    for caps in ((v - 1, 2 * f), (2 * v, f - 1), (3, 3)):
        del calls[:]
        monkeypatch.setattr(fusion.TSDFVolume, '_mesh_capacities', lambda self: caps)
        assert_mesh_equal(vol.extract_mesh(min_weight), want)
        assert calls == [caps, (v, f)]                                                   # the second run, at exactly (V, F)
    with pytest.raises(ValueError, match='mesh_device'):
        real(*dev, vertex_capacity=4, face_capacity=4, faces=torch.zeros(4, 3, dtype=torch.int64, device=DEV), **grid)
    with pytest.raises(ValueError, match='mesh_device'):
        real(dev[0].cpu(), dev[1], dev[2], vertex_capacity=4, face_capacity=4, **grid)


# ------------------------------------------------------------------ 5. more workgroups than scan threads
def test_long_scan():
    # 294912 voxels: 1152 workgroups of 256 against the 1024 threads of the scan workgroup, so each thread walks a run of two counts
    dims = (96, 64, 48)
    t, w, col = (v.float() for v in mu.sphere_volume(dims, 0.02, np.array([47.3, 31.6, 23.2]) * 0.02, 20.4 * 0.02, seed=4))
    grid = dict(origin=(-1.0, -0.7, 1.2), voxel=0.02)
    want = fusion.extract_mesh_host(t, w, col, **grid)
    assert want[0].shape[0] > 20000 and -(-dims[0] * dims[1] * dims[2] // 256) > 1024
    got = on_device(t, w, col, grid).extract_mesh()
    assert_mesh_equal(got, want)
    per_edge, repeats, edges = mu.topology(got[2].cpu().numpy())
    assert per_edge == {2} and repeats == 1 and got[0].shape[0] - edges + got[2].shape[0] == 2
    empty = on_device(torch.zeros_like(t), torch.zeros_like(w), None, grid).extract_mesh()
    assert [tuple(v.shape) for v in (empty[0], empty[2])] == [(0, 3)] * 2 and empty[1] is None


# ------------------------------------------------------------------ 6. memory contract
def test_memory_contract():
    t, w, col, grid, min_weight = volume(2)

    def fresh():
        geometry._hip_ops = None               # the module's own HipOps: a fresh one per run

    def run(_, g):
        nz, ny, nx = t.shape
        vol = fusion.TSDFVolume(grid['origin'], grid['voxel'], (nx, ny, nz), device=DEV)
        vol.tsdf, vol.weight, vol.color = g.place(t), g.place(w), g.place(col)           # read only: the guard checks they keep their bytes
        xyz, rgb, faces = vol.extract_mesh(min_weight)
        assert faces.shape[0] > 800
        small = fusion.mesh_device(vol.tsdf, vol.weight, vol.color, min_weight=min_weight, vertex_capacity=100, face_capacity=50, **grid)
        return xyz, rgb, faces, small[3], small[0], small[1], small[2]

    try:
        first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=fresh)
    finally:
        geometry._hip_ops = None
    assert any('fusion.py' in site for site in mg.contract.last_sites)
    want = host_mesh(2)
    assert torch.equal(first[0], want[0].reshape(-1).view(torch.uint8)) and torch.equal(first[1], want[1].reshape(-1))
    assert torch.equal(first[2], want[2].int().reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------ 7. invalid values reach nothing
def test_invalid_values_reach_nothing():
    t, w, col, grid, min_weight = volume(2)
    t, w, col = t.clone(), w.clone(), col.clone()
    g = torch.Generator().manual_seed(23)
    bad = torch.randint(0, 60, t.shape, generator=g)
    for code, value in ((1, float('nan')), (2, float('inf')), (3, -float('inf')), (4, 1.0), (5, -1.0), (6, 1.5)):
        t[bad == code] = value
    w[bad == 7] = 0.0
    w[bad == 8] = float('nan')
    col[:, bad == 9] = float('nan')                                                      # a colour without a value: 0, and the voxel stays valid
    want = fusion.extract_mesh_host(t, w, col, min_weight=min_weight, **grid)
    assert 300 < want[2].shape[0] < host_mesh(2)[2].shape[0]
    got = tuple(v.cpu() for v in on_device(t, w, col, grid).extract_mesh(min_weight))
    assert_mesh_equal(got, want)
    assert torch.isfinite(got[0]).all()
    # no vertex on an edge that touches an invalid voxel, so no face does either: every face indexes a vertex
    invalid = ~((w >= min_weight) & (t.abs() < 1))
    _, sel = fusion.mesh_edges_host(t, w, min_weight)
    k, j, i, a = sel.nonzero(as_tuple=True)
    e = a + 1
    assert not invalid[k, j, i].any() and not invalid[k + (e >> 2 & 1), j + (e >> 1 & 1), i + (e & 1)].any()
    assert int(got[2].min()) >= 0 and int(got[2].max()) < got[0].shape[0] and len(torch.unique(got[2])) == got[0].shape[0]
    per_edge, repeats, _ = mu.topology(got[2].numpy())
    assert per_edge <= {1, 2} and repeats == 1
