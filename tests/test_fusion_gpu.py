"""GPU tests of the TSDF fusion: ``um_tsdf_integrate`` and ``um_tsdf_points`` (csrc/fusion.hip) against the float64 evaluation of the
definition and, BITWISE, against the float32 host restatement of ``unimatch_amd/fusion.py``.

The three cases of tests/fusion_util.py (nx = 37, 40, 48: ragged against 64-wide waves; 24679 to 69120 voxels: many 256-thread
workgroups with a ragged last one), 1, 3 and 4 views, with weights and colours.  The margins of the float64 comparison come from the two
host evaluations (float32 against float64), never from the kernel; the host results are computed once per case and shared.  One larger
volume (130 x 70 x 40: 1422 workgroups, so the single scan workgroup walks runs of two counts) and one checkerboard volume (more
crossings than the first capacity of ``extract_points``: the second run) cover the remaining paths of the extraction."""
import numpy as np
import pytest
import torch

from unimatch_amd import fusion, geometry
from tests import fusion_util as fu
from tests import memory_guard as mg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASE_IDS = [1, 2, 3]
_device_results = {}


def integrate_on_device(c, weighted=True, color=True, one_by_one=False):
    """The case through ``um_tsdf_integrate``: ``(tsdf, weight, color)`` on the device."""
    t, w, col = (None if v is None else v.to(DEV) for v in c.volume(torch.float32, color))
    depth, cam, wi, rgb = c.depth.to(DEV), c.cam_view.to(DEV), c.weight_in.to(DEV), c.colors.to(DEV)
    for lo, hi in ([(i, i + 1) for i in range(c.views)] if one_by_one else [(0, c.views)]):
        fusion.integrate_device(t, w, col, depth[lo:hi].contiguous(), cam[lo:hi].contiguous(), wi[lo:hi].contiguous() if weighted else None,
                                rgb[lo:hi].contiguous() if color else None, **c.kw)
    return t, w, col


def device_result(number):
    if number not in _device_results:
        _device_results[number] = tuple(v.cpu() for v in integrate_on_device(fu.case(number)))
    return _device_results[number]


def assert_same(got, want, what=''):
    for name, g, h in zip(('tsdf', 'weight', 'color'), got, want):
        if h is None:
            assert g is None
            continue
        g, h = g.cpu(), h.cpu()
        same = g.view(torch.int32) == h.view(torch.int32)
        assert bool(same.all()), f'{what}{name}: {int((~same).sum())} of {same.numel()} values differ, the largest by {float((g - h).abs().max())}'


# ------------------------------------------------------------------ 1. device against float64
@pytest.mark.parametrize('number', CASE_IDS)
def test_device_against_float64(number):
    c = fu.case(number)
    t, w, col = device_result(number)
    t64, w64, c64 = c.host64
    err = float((t.double() - t64)[c.decided].abs().max())
    print(f'case {number}: device |tsdf - tsdf64| on decided voxels {err:.3g}, margin {c.tsdf_margin:.3g}, undecided {c.undecided_share:.5f}')
    assert c.undecided_share <= 0.01
    assert torch.equal(w.double()[c.decided], w64[c.decided])
    assert err <= c.tsdf_margin
    assert torch.isfinite(t).all() and torch.isfinite(col).all()


# ------------------------------------------------------------------ 2. device against the float32 restatement: bitwise
@pytest.mark.parametrize('number', CASE_IDS)
def test_device_bitwise_against_host(number):
    c = fu.case(number)
    assert_same(device_result(number), c.host32)
    assert float((c.host32[1] > 0).float().mean()) > 0.25 and c.host32[2].max() > 200


# ------------------------------------------------------------------ 3. one B-view call equals B one-view calls
@pytest.mark.parametrize('number', [2, 3])
def test_sequential_equivalence(number):
    assert_same(integrate_on_device(fu.case(number), one_by_one=True), device_result(number))


# ------------------------------------------------------------------ 4. extraction on the device-produced volume
@pytest.mark.parametrize('number', CASE_IDS)
def test_extraction_on_device_volume(number):
    c = fu.case(number)
    t, w, col = device_result(number)
    for min_weight in (0.5, 1.0, float(c.views)):
        want_xyz, want_rgb = fusion.extract_points_host(t, w, col, min_weight=min_weight, **c.grid)       # on the same bytes
        n = want_xyz.shape[0]
        xyz, rgb, count = fusion.points_device(t.to(DEV), w.to(DEV), col.to(DEV), min_weight=min_weight, capacity=n + 3, **c.grid)
        assert int(count.item()) == n and (n > 100 or min_weight > 1)
        # selection and order: every row is the crossing the host finds at that rank -- each coordinate within one subtraction, one
        # division, one product and one sum of the float64 evaluation of the same stored values (the voxel centre is a float32 value
        # by definition: its own product and sum are not part of the error)
        ref, ref_rgb, where = fu.points_loop(t, w, col, fu.ORIGIN, c.voxel, min_weight, centre=np.float32)
        assert len(where) == n
        got = xyz[:n].cpu()
        bound = 8 * 2.0 ** -24 * (np.abs(ref) + float(np.float32(c.voxel)))
        assert (np.abs(got.double().numpy() - ref) <= bound).all()
        assert torch.equal(got, want_xyz)                                                # and bit for bit what the restatement gives
        assert torch.equal(rgb[:n].cpu(), want_rgb)
        if n < 2:
            continue
        # capacity = N - 1: count still receives N, row N - 1 stays untouched
        buf = torch.full((n, 3), -777.0, device=DEV)
        buf_rgb = torch.full((n, 3), 93, dtype=torch.uint8, device=DEV)
        _, _, count = fusion.points_device(t.to(DEV), w.to(DEV), col.to(DEV), min_weight=min_weight, capacity=n - 1, xyz=buf[:n - 1],
                                           rgb=buf_rgb[:n - 1], **c.grid)
        assert int(count.item()) == n
        assert torch.equal(buf[:n - 1].cpu(), want_xyz[:n - 1]) and torch.equal(buf_rgb[:n - 1].cpu(), want_rgb[:n - 1])
        assert bool((buf[n - 1] == -777.0).all()) and bool((buf_rgb[n - 1] == 93).all())


def test_extract_points_second_run_and_long_scan():
    # a checkerboard: every edge of the volume crosses, more points than the first capacity 6 (nx ny + ny nz + nx nz)
    nx, ny, nz = 9, 8, 10
    k, j, i = torch.meshgrid(torch.arange(nz), torch.arange(ny), torch.arange(nx), indexing='ij')
    vol = fusion.TSDFVolume((0.5, -1.0, 2.0), 0.25, (nx, ny, nz), device=DEV)
    sign = (1 - 2 * ((i + j + k) % 2)).float()
    g = torch.Generator().manual_seed(5)
    vol.tsdf.copy_(sign * (0.05 + 0.9 * torch.rand(nz, ny, nx, generator=g)))
    vol.weight.fill_(1.0)
    vol.color.copy_(torch.rand(3, nz, ny, nx, generator=g) * 255)
    xyz, rgb = vol.extract_points()
    n = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    assert xyz.shape[0] == n > 6 * (nx * ny + ny * nz + nx * nz)
    want_xyz, want_rgb = fusion.extract_points_host(vol.tsdf.cpu(), vol.weight.cpu(), vol.color.cpu(), origin=vol.origin, voxel=vol.voxel_size)
    assert torch.equal(xyz.cpu(), want_xyz) and torch.equal(rgb.cpu(), want_rgb)
    vol.reset()
    assert vol.extract_points()[0].shape[0] == 0 and not vol.tsdf.any()
    # 364000 voxels: 1422 workgroups of 256, so every thread of the scan workgroup walks a run of two counts
    c = fu.case(1)
    big = fusion.TSDFVolume((-1.0, -0.7, 1.2), 0.02, (130, 70, 40), with_color=False, device=DEV)
    big.integrate(c.depth.to(DEV), c.k.to(DEV), c.poses.to(DEV), min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    host = fusion.TSDFVolume((-1.0, -0.7, 1.2), 0.02, (130, 70, 40), with_color=False, device='cpu')
    host.integrate(c.depth, c.k, c.poses, min_depth=fu.MIN_DEPTH, max_depth=fu.MAX_DEPTH)
    assert_same((big.tsdf, big.weight, None), (host.tsdf, host.weight, None), 'big: ')
    xyz, none = big.extract_points()
    assert none is None and xyz.shape[0] > 2000 and torch.equal(xyz.cpu(), host.extract_points()[0])
    assert (fu.surface_distance(xyz.double().cpu().numpy()) / 0.02).max() <= 1.0


# ------------------------------------------------------------------ 5. optional inputs
@pytest.mark.parametrize('weighted, color', [(False, True), (True, False), (False, False)])
def test_optional_inputs(weighted, color):
    c = fu.case(2)
    got = integrate_on_device(c, weighted=weighted, color=color)
    want = c.evaluate(torch.float32, weighted=weighted, color=color)
    assert_same(got, want)
    xyz, rgb, count = fusion.points_device(*got, capacity=4000, **c.grid)
    want_xyz, want_rgb = fusion.extract_points_host(*want, **c.grid)
    n = int(count.item())
    assert n == want_xyz.shape[0] > 100 and torch.equal(xyz[:n].cpu(), want_xyz)
    assert (rgb is None and want_rgb is None) if not color else torch.equal(rgb[:n].cpu(), want_rgb)


# ------------------------------------------------------------------ 6. memory contract
def test_memory_contract():
    c = fu.case(2)

    def fresh():
        geometry._hip_ops = None               # the module's own HipOps: a fresh one per run

    def run(_, g):
        vol = fusion.TSDFVolume(fu.ORIGIN, c.voxel, c.dims, device=DEV)
        vol.tsdf, vol.weight, vol.color = (g.place(t, inout=True) for t in c.volume(torch.float32))     # the in / out state
        depth, k, poses = g.place(c.depth), g.place(c.k), g.place(c.poses)
        weight, colors = g.place(c.weight_in), g.place(c.colors)
        vol.integrate(depth[:2], k, poses[:2], weight[:2], colors[:2], fu.MIN_DEPTH, fu.MAX_DEPTH)
        vol.integrate(depth[2:], k, poses[2:], weight[2:], colors[2:], fu.MIN_DEPTH, fu.MAX_DEPTH)
        xyz, rgb = vol.extract_points(0.5)
        assert xyz.shape[0] > 100
        return vol.tsdf, vol.weight, vol.color, xyz, rgb

    try:
        first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=fresh)
    finally:
        geometry._hip_ops = None
    assert any('fusion.py' in site for site in mg.contract.last_sites)
    want = c.host32
    for got, h in zip(first[:3], want):
        assert torch.equal(got, h.reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------ 7. invalid values: the clamped-address contract
def test_invalid_values_reach_nothing():
    c = fu.case(3)
    b, h, w = c.views, c.h, c.w
    g = torch.Generator().manual_seed(9)
    depth = c.depth.clone()
    bad = torch.randint(0, 8, (b, h, w), generator=g)
    for code, value in ((1, float('nan')), (2, float('inf')), (3, 1e30), (4, -float('inf')), (5, -1.0)):
        depth[bad == code] = value
    k = c.k.expand(b, 3, 3).clone()
    k[1, 2] = 0.0                                                                        # a singular intrinsics row: view 1 sees nothing
    poses = c.poses.clone()
    poses[2, 0, 3] = float('nan')                                                        # and view 2 has no position
    dev = fusion.TSDFVolume(fu.ORIGIN, c.voxel, c.dims, device=DEV)
    dev.integrate(depth.to(DEV), k.to(DEV), poses.to(DEV), c.weight_in.to(DEV), c.colors.to(DEV), fu.MIN_DEPTH, fu.MAX_DEPTH)
    host = fusion.TSDFVolume(fu.ORIGIN, c.voxel, c.dims, device='cpu')
    host.integrate(depth, k, poses, c.weight_in, c.colors, fu.MIN_DEPTH, fu.MAX_DEPTH)
    got = (dev.tsdf.cpu(), dev.weight.cpu(), dev.color.cpu())
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert_same(got, (host.tsdf, host.weight, host.color))
    # what the two valid views reached through their valid pixels, and nothing elsewhere
    valid = torch.tensor([0, 3])
    weight = torch.where((bad[valid] == 0) | (bad[valid] > 5), c.weight_in[valid], torch.zeros(()))       # codes 6, 7: left valid
    only = fusion.TSDFVolume(fu.ORIGIN, c.voxel, c.dims, device='cpu')
    only.integrate(c.depth[valid], c.k, c.poses[valid], weight, c.colors[valid], fu.MIN_DEPTH, fu.MAX_DEPTH)
    assert_same(got, (only.tsdf, only.weight, only.color))
    untouched = got[1] == 0
    assert 0.2 < float(untouched.float().mean()) < 0.9 and not got[0][untouched].any() and not got[2][:, untouched].any()
    xyz, rgb = dev.extract_points(0.5)
    assert torch.isfinite(xyz).all() and torch.equal(xyz.cpu(), host.extract_points(0.5)[0])
