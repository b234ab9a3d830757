"""GPU tests of ``um_disp_consistency``, ``um_depth_consistency`` and ``um_points_pack`` against fp64 evaluations, the reference
fixtures, and the host path of :mod:`unimatch_amd.geometry`.

Depth consistency is held to margins that are computed per case and per quantity from two HOST evaluations, never from the kernel:
4 x the largest ``|fp32 host - fp64|`` over the case's finite pixels (``tests/geometry_util.margins``).  Measured for the four cases
below (px, relative): (3,33,47) 5.8e-5, 9.2e-6 | (2,64,97) 1.2e-4, 1.4e-5 | (1,5,3) 9.7e-7, 5.4e-7 | (1,16,64) 5.2e-5, 6.4e-6.  The
relative margins are larger than the noise alone would give (about 1e-6) because the scaled block puts a 50 % depth step between
neighbouring source pixels: a coordinate that differs by 3e-5 px samples a depth that differs by 1.5e-5 there."""
import os

import numpy as np
import pytest
import torch

from unimatch_amd import geometry
from unimatch_amd.ops import HipOps
from tests import geometry_util as gu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'geometry.npz')
SEEDS = (101, 102, 103, 104)


@pytest.fixture(scope='module')
def ops():
    return HipOps()


# ------------------------------------------------------------------ disparity
@pytest.mark.parametrize('seed,shape', list(zip(SEEDS, gu.SHAPES)))
def test_disp_consistency_against_fp64(seed, shape):
    dl, dr = gu.disparity_pair(seed, *shape)
    for alpha, beta in ((0.01, 0.5), (0.05, 0.1)):
        occ_l, occ_r = geometry.disparity_consistency_check(dl.to(DEV), dr.to(DEV), alpha, beta)
        assert occ_l.is_cuda and occ_l.dtype == torch.float32 and occ_l.shape == dl.shape
        ml, mr, thr = gu.occ_margins(*gu.disparity_flows(dl, dr), alpha, beta)
        gu.check_occ(occ_l, (ml > 0).float(), ml, thr)
        gu.check_occ(occ_r, (mr > 0).float(), mr, thr)
        host_l, host_r = geometry.disparity_consistency_check(dl, dr, alpha, beta)
        gu.check_occ(occ_l, host_l, ml, thr)                                              # the host path: the same operations in fp32
        gu.check_occ(occ_r, host_r, mr, thr)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_disp_consistency_matches_reference(tag):
    g = np.load(GOLDEN)
    dl, dr = torch.from_numpy(g[f'disp_left_{tag}']), torch.from_numpy(g[f'disp_right_{tag}'])
    occ_l, occ_r = geometry.disparity_consistency_check(dl.to(DEV), dr.to(DEV))
    ml, mr, thr = gu.occ_margins(*gu.disparity_flows(dl, dr))
    gu.check_occ(occ_l, torch.from_numpy(g[f'occ_left_{tag}']), ml, thr)
    gu.check_occ(occ_r, torch.from_numpy(g[f'occ_right_{tag}']), mr, thr)


# ------------------------------------------------------------------ depth consistency
@pytest.mark.parametrize('seed,shape', list(zip(SEEDS, gu.SHAPES)))
def test_depth_consistency_against_fp64(seed, shape):
    ref, src, k, pose = gu.plane_pair(seed, *shape)
    f64, f32 = gu.depth_check_fp64(ref, src, k, pose), gu.depth_check_fp32(ref, src, k, pose)
    margin = gu.margins(f32, f64)
    got = geometry.depth_consistency_check(ref.to(DEV), src.to(DEV), k.to(DEV), pose.to(DEV), return_errors=True)
    assert all(t.is_cuda and t.dtype == torch.float32 and t.shape == ref.shape for t in got)
    print(shape, 'margins', margin, 'max |device - fp64|', [(a.cpu().double() - b)[torch.isfinite(b)].abs().max().item()
                                                            for a, b in zip(got[1:], f64[1:])])
    off_host = gu.check_depth_result(f32, f64, margin)
    off_dev = gu.check_depth_result(got, f64, margin)
    print(shape, 'mask pixels off fp64: host', off_host, 'device', off_dev)
    occ_only = geometry.depth_consistency_check(ref.to(DEV), src.to(DEV), k[:1].to(DEV), pose.to(DEV))          # null error outputs
    assert torch.equal(occ_only, got[0])


# ------------------------------------------------------------------ points
def xyz_close(got, want):
    """Rows within 1e-5 max(1, max |xyz|) of fp64: about ten fp32 operations at half an ulp of the largest intermediate, times 16."""
    return got.shape[0] == 0 or (got.cpu().double() - want).abs().max() <= 1e-5 * max(1.0, want.abs().max().item())


def points_case(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    depth = (1.0 + 3.0 * torch.rand(b, h, w, generator=g)).float()
    flat = depth.view(-1)
    flat[0], flat[flat.numel() // 2], flat[-1] = float('nan'), float('inf'), -2.0
    keep = (torch.rand(b, h, w, generator=g) < 0.4).float()
    colors = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    k = gu.intrinsics_for(h, w).float()[None]
    poses = torch.stack([gu.rigid((0.3, 1.0, -0.2), 0.1 + 0.2 * i, (0.5 * i, -0.2, 0.1 * i)) for i in range(b)], 0).float()
    return depth, keep, colors, k, poses


def points_fp64(depth, keep, colors, k, poses, lo, hi, stride):
    sel = geometry.points_selection_host(depth, keep, lo, hi, stride)
    cam = gu.cam_fp64(k.expand(depth.shape[0], 3, 3), poses)[0]
    gx, gy = geometry._pixel_grid(depth.shape[1], depth.shape[2], torch.float64)
    xyz = torch.stack(geometry._lift(cam, gx, gy, torch.where(sel, depth, torch.zeros_like(depth)).double()), -1)
    idx = torch.nonzero(sel)                                          # ascending (b, y, x)
    return xyz[idx[:, 0], idx[:, 1], idx[:, 2]], None if colors is None else colors[idx[:, 0], idx[:, 1], idx[:, 2]]


@pytest.mark.parametrize('seed,shape', list(zip(SEEDS, gu.SHAPES)))
def test_points_pack_order_and_values(seed, shape):
    depth, keep, colors, k, poses = points_case(seed, *shape)
    dev = [t.to(DEV) for t in (depth, keep, colors, k, poses)]
    for stride in (1, 3):
        for kp, col in ((keep, colors), (None, colors), (keep, None), (None, None)):
            want_xyz, want_rgb = points_fp64(depth, kp, col, k, poses, 1.5, 3.5, stride)
            xyz, rgb = geometry.back_project_points(dev[0], dev[3], dev[4], keep=None if kp is None else dev[1],
                                                    colors=None if col is None else dev[2], min_depth=1.5, max_depth=3.5, stride=stride)
            assert xyz.is_cuda and xyz.dtype == torch.float32 and tuple(xyz.shape) == tuple(want_xyz.shape)      # N ...
            assert xyz_close(xyz, want_xyz)                                                                      # ... and the row order
            assert (rgb is None) == (col is None) and (col is None or torch.equal(rgb.cpu(), want_rgb))
    none = geometry.back_project_points(dev[0], dev[3], dev[4], keep=torch.zeros_like(dev[1]), colors=dev[2])
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)


def test_points_pack_workspace_carries_nothing_over(ops):
    """Two geometries through one HipOps, the larger first: were a count or an offset of the first call read by the second, its rows
    would move."""
    big, small = points_case(7, 2, 64, 97), points_case(8, 3, 33, 47)
    for depth, keep, colors, k, poses in (big, small, big):
        cam = ops.depth_cam(k.expand(depth.shape[0], 3, 3).contiguous().to(DEV), poses.to(DEV), 1.0)
        xyz, rgb, count = ops.points_pack(depth.to(DEV), cam, keep.to(DEV), colors.to(DEV), 0.0, 3.0, 1)
        want_xyz, want_rgb = points_fp64(depth, keep, colors, k, poses, 0.0, 3.0, 1)
        n = int(count.item())
        assert n == want_xyz.shape[0] and torch.equal(rgb[:n].cpu(), want_rgb)
        assert n > 1000 and xyz_close(xyz[:n], want_xyz)
    with pytest.raises(ValueError):
        ops.points_pack(depth.to(DEV), cam[:1], None, None)
    with pytest.raises(ValueError):
        ops.points_pack(depth.to(DEV), cam, keep.to(DEV)[:, :2], None)
    with pytest.raises(ValueError):
        ops.disp_consistency(depth.to(DEV), depth.to(DEV)[:, :, :1])
    with pytest.raises(ValueError):
        ops.depth_consistency(depth.to(DEV), depth.to(DEV), cam, cam[:1])


# ------------------------------------------------------------------ end to end
def test_fuse_depth_sequence_device_equals_host():
    from tests.test_geometry_cpu import plane_sequence
    t, h, w = 4, 33, 47
    depths, k, poses, _ = plane_sequence(t, h, w)
    g = torch.Generator().manual_seed(9)
    depths = depths * (1 + 0.004 * torch.randn(t, h, w, generator=g))
    colors = torch.randint(0, 256, (t, h, w, 3), generator=g, dtype=torch.uint8)
    host = geometry.fuse_depth_sequence(depths, k, poses, colors)
    dev = geometry.fuse_depth_sequence(depths.to(DEV), k.to(DEV), poses.to(DEV), colors.to(DEV))
    assert dev['xyz'].is_cuda and dev['keep'].shape == (t, h, w) and dev['xyz'].shape[0] == int(dev['keep'].sum()) == dev['rgb'].shape[0]
    assert 0.1 < host['keep'].mean() < 0.95
    # keep under the margin rule: the 2 (T - 1) directed checks in fp32 and fp64 on the host give the margins
    rel = geometry.relative_pose_pairs_host(poses)
    ref, src = torch.cat([depths[:-1], depths[1:]], 0), torch.cat([depths[1:], depths[:-1]], 0)
    pose2, k2 = torch.cat([rel, torch.linalg.inv(rel.double()).float()], 0), k.expand(2 * (t - 1), 3, 3)
    f64, f32 = gu.depth_check_fp64(ref, src, k2, pose2), gu.depth_check_fp32(ref, src, k2, pose2)
    margin = gu.margins(f32, f64)
    near = ((f64[1] - 1.0).abs() <= margin[0]) | ((f64[2] - 0.01).abs() <= margin[1])
    near_frame = torch.zeros(t, h, w, dtype=torch.bool)
    near_frame[:-1] |= near[:t - 1]
    near_frame[1:] |= near[t - 1:]
    off = dev['keep'].cpu() != host['keep']
    assert not (off & ~near_frame).any() and int(off.sum()) <= 0.005 * off.numel()
    # rows compared one to one on the pixels both keep
    both = (dev['keep'].cpu() == 1) & (host['keep'] == 1)
    rows_dev, rows_host = both[dev['keep'].cpu() == 1], both[host['keep'] == 1]
    a, b = dev['xyz'].cpu()[rows_dev], host['xyz'][rows_host]
    assert a.shape == b.shape and a.shape[0] > 1000 and xyz_close(a, b.double())
    assert torch.equal(dev['rgb'].cpu()[rows_dev], host['rgb'][rows_host])
