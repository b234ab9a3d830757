"""CPU tests of the consistency masks and point clouds: the host restatements of :mod:`unimatch_amd.geometry` against fixtures minted
from the reference (``tests/golden/make_golden_geometry.py``), the C ABI of the four new entry points without a GPU, the PLY codec,
``fuse_depth_sequence`` on an analytic plane scene, and the two runners' new flags with stand-in models of their own."""
import ctypes
import os

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, geometry, io
from unimatch_amd.prepost import InferenceGeometry
from tests import geometry_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'geometry.npz')


@pytest.fixture(scope='module')
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


# ------------------------------------------------------------------ 1. the host restatements against the reference's results
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_host_reprojection_matches_reference(golden, tag):
    depth, k, pose = golden[f'depth_{tag}'], golden[f'k_{tag}'], golden[f'pose_{tag}']
    b, h, w = depth.shape
    cam = geometry.cam_pack_host(k, pose, bidir=True)
    assert cam.shape == (2 * b, 30) and cam.dtype == torch.float32
    gx, gy = geometry._pixel_grid(h, w, torch.float32)
    ident = geometry.cam_pack_host(k, torch.eye(4)[None].repeat(b, 1, 1))
    points = torch.stack(geometry._lift(ident, gx, gy, depth), 1)                   # back_project
    moved = torch.stack(geometry._lift(cam[:b], gx, gy, depth), 1)                  # ... and camera_transform
    for got, name in ((points, 'points'), (moved, 'moved')):
        want = golden[f'{name}_{tag}']
        assert (got - want).abs().max() <= 1e-5 * max(1.0, want.abs().max().item()), name
    u, v, mask = geometry.reproject_host(depth, cam[:b])
    want = golden[f'coords_{tag}']
    assert (u - want[:, 0]).abs().max() <= 1e-4 and (v - want[:, 1]).abs().max() <= 1e-4
    off = mask != golden[f'mask_{tag}'].bool()
    border = torch.minimum(torch.minimum(want[:, 0].abs(), (want[:, 0] - (w - 1)).abs()),
                           torch.minimum(want[:, 1].abs(), (want[:, 1] - (h - 1)).abs()))
    assert (border[off] <= 1e-4).all()
    assert 0.02 < golden[f'mask_{tag}'].float().mean() < 0.98                        # the fixture has both classes
    # the second half of the pack is the inverse pose
    rel = torch.eye(4)[None].repeat(b, 1, 1)
    rel[:, :3, :3], rel[:, :3, 3] = cam[b:, 9:18].view(b, 3, 3), cam[b:, 18:21]
    assert (rel.double() @ pose.double() - torch.eye(4, dtype=torch.float64)).abs().max() <= 1e-6


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_host_disparity_check_matches_reference(golden, tag):
    dl, dr = golden[f'disp_left_{tag}'], golden[f'disp_right_{tag}']
    occ_l, occ_r = geometry.disparity_consistency_check(dl, dr)
    assert occ_l.dtype == torch.float32 and occ_l.shape == dl.shape
    ml, mr, thr = gu.occ_margins(*gu.disparity_flows(dl, dr))
    gu.check_occ(occ_l, golden[f'occ_left_{tag}'], ml, thr)
    gu.check_occ(occ_r, golden[f'occ_right_{tag}'], mr, thr)
    for occ in (golden[f'occ_left_{tag}'], golden[f'occ_right_{tag}']):
        assert 0.05 < occ.float().mean() < 0.95
    # the two-tap restatement IS the flow check on (-dL, 0) / (dR, 0): the four-tap host evaluation gives the same masks
    from unimatch_amd.video import forward_backward_consistency_check
    f4, b4 = forward_backward_consistency_check(*gu.disparity_flows(dl, dr))
    gu.check_occ(occ_l, f4, ml, thr)
    gu.check_occ(occ_r, b4, mr, thr)


def test_disparity_check_properties():
    dl = torch.full((1, 4, 16), 3.0)
    occ_l, occ_r = geometry.disparity_consistency_check(dl, dl.clone())
    # a constant disparity agrees wherever the match is in frame; the first (last) three columns match outside: zeros are sampled
    assert torch.equal(occ_l[0, 0], torch.tensor([1.] * 3 + [0.] * 13)) and torch.equal(occ_r[0, 0], torch.tensor([0.] * 13 + [1.] * 3))
    one_row = geometry.disparity_consistency_check(dl[:, :1], dl[:, :1].clone())          # H = 1 is fine: only W >= 2 is needed
    assert torch.equal(one_row[0], occ_l[:, :1])
    nan = dl.clone()
    nan[0, 1, 5] = float('nan')
    assert torch.isfinite(geometry.disparity_consistency_check(nan, dl)[0]).all()
    for bad in ((dl[0], dl[0]), (dl, dl[:, :2]), (dl[..., :1], dl[..., :1])):
        with pytest.raises(ValueError):
            geometry.disparity_consistency_check(*bad)


def test_host_depth_check_classes_and_fp32_against_fp64():
    """The test scenes hold every class, and the fp32 restatement agrees with fp64 under the rule the kernel is held to."""
    for seed, (b, h, w) in zip((101, 102, 103, 104), gu.SHAPES):
        ref, src, k, pose = gu.plane_pair(seed, b, h, w)
        f64, f32 = gu.depth_check_fp64(ref, src, k, pose), gu.depth_check_fp32(ref, src, k, pose)
        margin = gu.margins(f32, f64)
        assert 0 < margin[0] < 1e-3 and 0 < margin[1] < 1e-4, margin             # a sanity bound; the margins are whatever the two evaluations give
        gu.check_depth_result(f32, f64, margin)
        occ, epx, erel = f64
        n = occ.numel()
        if h * w >= 64:
            shares = (torch.isinf(epx).sum() / n, (occ == 0).sum() / n, (torch.isfinite(epx) & (epx >= 1.0)).sum() / n,
                      (torch.isfinite(erel) & (erel >= 0.01)).sum() / n)
            assert all(s >= 0.02 for s in shares), (h, w, shares)
        else:
            fin = torch.isfinite(epx)
            assert ((epx[fin] - 1.0).abs() >= 100 * margin[0]).all() and ((erel[fin] - 0.01).abs() >= 100 * margin[1]).all()
    occ = geometry.depth_consistency_check(ref, src, k[:1], pose)                         # public function, shared intrinsics
    assert torch.equal(occ, f32[0])
    out = geometry.depth_consistency_check(ref, src, k, pose, return_errors=True)
    assert len(out) == 3 and torch.equal(out[1], f32[1])
    with pytest.raises(ValueError):
        geometry.depth_consistency_check(ref, src, k, pose[0])
    with pytest.raises(ValueError):
        geometry.depth_consistency_check(ref, src[:, :2], k, pose)


# ------------------------------------------------------------------ 2. the C ABI without a GPU
DECLARATIONS = {
    'um_disp_consistency': 'int um_disp_consistency(const float* disp_left, const float* disp_right, float* occ_left, float* occ_right, '
                           'int batch, int h, int w, float alpha, float beta, void* stream);',
    'um_depth_consistency': 'int um_depth_consistency(const float* depth_ref, const float* depth_src, const float* cam_fwd, '
                            'const float* cam_inv, float* occ, float* err_px, float* err_rel, int batch, int h, int w, float px_thr, '
                            'float rel_thr, void* stream);',
    'um_points_workspace_bytes': 'size_t um_points_workspace_bytes(int batch, int h, int w, int stride);',
    'um_points_pack': 'int um_points_pack(const float* depth, const float* cam_world, const float* keep, const unsigned char* colors, '
                      'float* xyz, unsigned char* rgb, int* count, int batch, int h, int w, int stride, float min_depth, float max_depth, '
                      'void* workspace, size_t ws_bytes, void* stream);',
}


def test_geometry_symbols_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = ' '.join(open(os.path.join(ROOT, 'include', 'unimatch_hip.h')).read().split())
    v, i, f, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    want = {'um_disp_consistency': (i, [v] * 4 + [i] * 3 + [f] * 2 + [v]),
            'um_depth_consistency': (i, [v] * 7 + [i] * 3 + [f] * 2 + [v]),
            'um_points_workspace_bytes': (z, [i] * 4),
            'um_points_pack': (i, [v] * 7 + [i] * 4 + [f] * 2 + [v, z, v])}
    for name, decl in DECLARATIONS.items():
        assert decl in text, name
        assert hasattr(lib, name) and _abi.SIGNATURES[name] == want[name], name
    from unimatch_amd.ops import HipOps
    assert callable(HipOps.disp_consistency) and callable(HipOps.depth_consistency) and callable(HipOps.points_pack)
    from unimatch_amd.build import EXTRA_FLAGS, SOURCES
    assert 'geometry.hip' in SOURCES and EXTRA_FLAGS['geometry.hip'] == EXTRA_FLAGS['metrics.hip']
    assert _abi.load().um_version() == 220


def test_geometry_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(16)
    for args in ((None, p, p, p, 1, 8, 8), (p, p, p, None, 1, 8, 8), (p, p, p, p, 0, 8, 8), (p, p, p, p, 1, 0, 8), (p, p, p, p, 1, 8, 1),
                 (p, p, p, p, 32768, 256, 256)):
        assert lib.um_disp_consistency(*args, 0.01, 0.5, None) == -1
        assert b'um_disp_consistency' in lib.um_last_error_string()
    for args in ((None, p, p, p, p, p, p, 1, 8, 8), (p, p, None, p, p, p, p, 1, 8, 8), (p, p, p, p, None, p, p, 1, 8, 8),
                 (p, p, p, p, p, None, None, 0, 8, 8), (p, p, p, p, p, None, None, 1, 8, -1), (p, p, p, p, p, p, p, 2, 32768, 32768)):
        assert lib.um_depth_consistency(*args, 1.0, 0.01, None) == -1
        assert b'um_depth_consistency' in lib.um_last_error_string()
    assert lib.um_points_workspace_bytes(2, 33, 47, 1) == 2 * 7 * 2 * 4                 # ceil(1551 / 256) counts and offsets per image
    assert lib.um_points_workspace_bytes(2, 33, 47, 3) == 2 * 7 * 2 * 4
    for bad in ((0, 8, 8, 1), (1, 8, 8, 0), (1, -8, 8, 1), (32768, 256, 256, 1)):
        assert lib.um_points_workspace_bytes(*bad) == 0
    tail = (1, 8, 8, 1, 0.0, 10.0, p, 1024, None)
    for head in ((None, p, p, p, p, p, p), (p, None, p, p, p, p, p), (p, p, p, p, None, p, p), (p, p, p, p, p, p, None),
                 (p, p, None, p, p, None, p), (p, p, None, None, p, p, p)):
        assert lib.um_points_pack(*head, *tail) == -1
        assert b'um_points_pack' in lib.um_last_error_string()
    assert lib.um_points_pack(p, p, None, None, p, None, p, 1, 8, 8, 0, 0.0, 10.0, p, 1024, None) == -1
    assert lib.um_points_pack(p, p, None, None, p, None, p, 1, 8, 8, 1, 0.0, 10.0, p, 4, None) == -3       # workspace too small
    assert lib.um_points_pack(p, p, None, None, p, None, p, 1, 8, 8, 1, 0.0, 10.0, None, 1024, None) == -3
    assert b'um_points_pack' in lib.um_last_error_string()


# ------------------------------------------------------------------ 3. PLY
def test_ply_round_trip_and_header_bytes(tmp_path):
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((7, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    path = str(tmp_path / 'cloud.ply')
    io.write_ply(path, xyz, rgb)
    blob = open(path, 'rb').read()
    header = (b'ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n'
              b'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    assert blob.startswith(header) and len(blob) == len(header) + 7 * 15 and blob.count(b'end_header') == 1
    assert blob[len(header):len(header) + 12] == xyz[0].astype('<f4').tobytes() and blob[len(header) + 12:len(header) + 15] == rgb[0].tobytes()
    got_xyz, got_rgb = io.read_ply(path)
    assert got_xyz.dtype == np.float32 and np.array_equal(got_xyz, xyz) and got_rgb.dtype == np.uint8 and np.array_equal(got_rgb, rgb)
    io.write_ply(path, xyz)                                                              # without colours: 12-byte rows
    blob = open(path, 'rb').read()
    assert b'red' not in blob and blob.endswith(xyz.astype('<f4').tobytes()) and blob.count(b'end_header') == 1
    got_xyz, got_rgb = io.read_ply(path)
    assert np.array_equal(got_xyz, xyz) and got_rgb is None
    io.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))         # an empty cloud is a header
    assert io.read_ply(path)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        io.write_ply(path, xyz[:, :2])
    with pytest.raises(ValueError):
        io.write_ply(path, xyz, rgb.astype(np.float32))
    open(path, 'wb').write(b'not a ply')
    with pytest.raises(ValueError):
        io.read_ply(path)


# ------------------------------------------------------------------ 4. fusing a plane seen from four poses
def plane_sequence(t, h, w, scale_frame=None):
    """``t`` camera-to-world poses looking at the world plane ``n . X = 2.5`` and the analytic depth map of each frame."""
    k = gu.intrinsics_for(h, w)
    normal = torch.tensor([0.1, -0.15, 1.0], dtype=torch.float64)
    normal = normal / normal.norm()
    poses = torch.stack([gu.rigid((0.1, 1.0, 0.2), 0.02 * i, (0.08 * i, -0.03 * i, 0.02 * i)) for i in range(t)], 0)
    depths = torch.stack([gu.plane_depth(*gu.plane_in(torch.linalg.inv(p), normal, 2.5), k, h, w) for p in poses], 0)
    if scale_frame is not None:
        depths[scale_frame] *= 1.2
    return depths.float(), k.float()[None], poses.float(), normal


def test_fuse_depth_sequence_on_a_plane():
    t, h, w = 4, 33, 47
    depths, k, poses, normal = plane_sequence(t, h, w, scale_frame=3)
    colors = torch.randint(0, 256, (t, h, w, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    out = geometry.fuse_depth_sequence(depths, k, poses, colors)
    keep, xyz, rgb = out['keep'], out['xyz'], out['rgb']
    assert keep.shape == (t, h, w) and xyz.shape == (int(keep.sum()), 3) and rgb.dtype == torch.uint8 and rgb.shape == xyz.shape
    assert keep[3].sum() == 0                                   # the frame whose depth is 20 % off agrees with nobody: no point
    assert keep[2].mean() > 0.8 and keep[1].mean() > 0.8        # frame 2 keeps what frame 1 confirms
    assert ((xyz.double() @ normal) - 2.5).abs().max() <= 1e-4 * 2.5
    assert torch.equal(rgb, colors[keep.bool()])               # rows in (t, y, x) order
    # min_views = 2: only pixels both neighbours confirm, so none of the end frames and none next to the bad frame
    two = geometry.fuse_depth_sequence(depths, k, poses, min_views=2)
    assert two['rgb'] is None and two['keep'][[0, 2, 3]].sum() == 0 and 0 < two['keep'][1].sum() <= keep[1].sum()
    # the point options reach the compaction: stride 3 keeps the pixels of every third row and column, a depth range cuts
    s3 = geometry.fuse_depth_sequence(depths, k, poses, colors, stride=3)
    grid = torch.zeros(h, w, dtype=torch.bool)
    grid[::3, ::3] = True
    assert torch.equal(s3['keep'], keep) and torch.equal(s3['rgb'], colors[keep.bool() & grid])
    cut = geometry.fuse_depth_sequence(depths, k, poses, min_depth=2.4, max_depth=2.6)
    assert cut['xyz'].shape[0] == int((keep.bool() & (depths > 2.4) & (depths < 2.6)).sum()) < xyz.shape[0]
    good = geometry.fuse_depth_sequence(*plane_sequence(t, h, w)[:3])
    assert good['keep'][3].mean() > 0.8
    with pytest.raises(ValueError):
        geometry.fuse_depth_sequence(depths[:1], k, poses[:1])
    with pytest.raises(ValueError):
        geometry.fuse_depth_sequence(depths, k, poses[:3])


def test_back_project_points_selection_and_order():
    depths, k, poses, _ = plane_sequence(2, 9, 11)
    depths[0, 2, 3], depths[1, 4, 4], depths[1, 0, 0] = float('nan'), float('inf'), -1.0
    keep = (torch.rand(2, 9, 11, generator=torch.Generator().manual_seed(2)) < 0.4).float()
    colors = torch.randint(0, 256, (2, 9, 11, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    xyz, rgb = geometry.back_project_points(depths, k, poses, keep=keep, colors=colors)
    sel = keep.bool() & torch.isfinite(depths) & (depths > 0)
    assert xyz.shape == (int(sel.sum()), 3) and torch.equal(rgb, colors[sel])
    cam = gu.cam_fp64(k.repeat(2, 1, 1), poses)[0]
    gx, gy = geometry._pixel_grid(9, 11, torch.float64)
    want = torch.stack(geometry._lift(cam, gx, gy, torch.where(sel, depths, torch.zeros_like(depths)).double()), -1)[sel]
    assert (xyz.double() - want).abs().max() <= 1e-5 * max(1.0, want.abs().max().item())
    assert geometry.back_project_points(depths, k, poses, keep=torch.zeros_like(depths))[0].shape == (0, 3)
    assert geometry.back_project_points(depths, k, poses)[1] is None
    for bad in (dict(stride=0), dict(keep=keep[:1]), dict(colors=colors.float())):
        with pytest.raises(ValueError):
            geometry.back_project_points(depths, k, poses, **bad)


# ------------------------------------------------------------------ 5. the runners, with stand-in models of their own
def read_png(path):
    from PIL import Image
    return np.array(Image.open(path))


class StereoStandIn:
    """``predict`` of the stereo runner: disparities that are a smooth function of the frames, the right view shifted to agree in part."""

    def predict(self, left, right, inference_size=None, pred_bidir_disp=False, **kw):
        n, h, w = left.shape[:3]
        base = 2.0 + 0.01 * left.float().mean(-1)
        x = torch.arange(w).view(1, 1, w).expand(n, h, w)
        right_view = base.gather(2, (x + 2).clamp(max=w - 1)) + (right.float().mean(-1) > 200) * 4.0
        return {'flow_preds': [torch.cat([base, right_view], 0) if pred_bidir_disp else base]}


def test_run_stereo_lr_check(tmp_path):
    pytest.importorskip('PIL')
    from unimatch_amd import stereo
    from unimatch_amd.video import read_frame_u8
    rng = np.random.default_rng(5)
    names = [f'{i:02d}_{side}.png' for i in range(2) for side in ('a', 'b')]
    os.makedirs(tmp_path / 'in')
    for name in names:
        io.write_png8(str(tmp_path / 'in' / name), rng.integers(0, 256, (20, 30, 3), dtype=np.uint8))
    lefts, rights = stereo.pair_lists(str(tmp_path / 'in'))
    model = StereoStandIn()
    stereo.run_stereo(model, lefts, rights, str(tmp_path / 'plain'), {}, pred_bidir_disp=True, batch_size=2, device='cpu')
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(f'{i:02d}_a{s}.png' for i in range(2) for s in ('_disp', '_disp_right'))
    stereo.run_stereo(model, lefts, rights, str(tmp_path / 'lr'), {}, pred_bidir_disp=True, batch_size=2, device='cpu', lr_check=True)
    assert sorted(os.listdir(tmp_path / 'lr')) == sorted(f'{i:02d}_a{s}.png' for i in range(2)
                                                         for s in ('_disp', '_disp_right', '_occ', '_occ_right'))
    for i in range(2):
        pred = model.predict(read_frame_u8(lefts[i])[None], read_frame_u8(rights[i])[None], pred_bidir_disp=True)['flow_preds'][-1]
        occ_l, occ_r = geometry.disparity_consistency_check(pred[:1], pred[1:])
        for suffix, occ in (('_occ', occ_l), ('_occ_right', occ_r)):
            png = read_png(str(tmp_path / 'lr' / f'{i:02d}_a{suffix}.png'))
            assert png.dtype == np.uint8 and set(np.unique(png)) == {0, 255} and np.array_equal(png, (occ[0].numpy() * 255).astype(np.uint8))
        assert np.array_equal(read_png(str(tmp_path / 'lr' / f'{i:02d}_a_disp.png')), read_png(str(tmp_path / 'plain' / f'{i:02d}_a_disp.png')))
    with pytest.raises(ValueError, match='pred-bidir-disp'):
        stereo.run_stereo(model, lefts, rights, str(tmp_path / 'x'), {}, device='cpu', lr_check=True)


H, W, T = 24, 40, 4


def write_plane_scene(root):
    """A ScanNet-layout scene whose poses and intrinsics are those of :func:`plane_sequence`; returns the analytic depths."""
    depths, k, poses, _ = plane_sequence(T, H, W)
    rng = np.random.default_rng(11)
    for sub in ('color', 'pose', 'intrinsic'):
        os.makedirs(root / sub)
    for i in range(T):
        io.write_png8(str(root / 'color' / f'{20 * i:04d}.png'), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        np.savetxt(str(root / 'pose' / f'{20 * i:04d}.txt'), poses[i].double().numpy())
    k4 = np.eye(4)
    k4[:3, :3] = k[0].double().numpy()
    np.savetxt(str(root / 'intrinsic' / 'intrinsic_depth.txt'), k4)
    return depths


class DepthStandIn:
    """Both entry points of the depth runner: the analytic plane depth of each frame (found through its pose), one percent off on the
    pixels whose red value is above 200, at whatever size the runner asks for."""

    def __init__(self, depths, poses):
        self.depths, self.poses, self.next = depths, poses, 0

    def _depth(self, i, frame_u8):
        return self.depths[i] * (1 + 0.05 * (frame_u8[..., 0] > 200))

    def predict(self, ref, tgt, inference_size=None, pred_bidir_depth=False, **kw):
        i, self.next = self.next, self.next + 1
        out = [self._depth(i, ref[0])] + ([self._depth(i + 1, tgt[0])] if pred_bidir_depth else [])
        return {'flow_preds': [torch.stack(out, 0)]}

    def forward_sequence(self, frames, carry=None, poses=None, pred_bidir_depth=False, **kw):
        # the prepared frames are at the inference size: the analytic depth goes there through the inverse of the runner's restore
        first = 0 if carry is None else carry['index']
        n = frames.shape[0] - (1 if carry is None else 0)
        geom = InferenceGeometry.resized((H, W), tuple(frames.shape[-2:]))
        up = lambda d: torch.nn.functional.interpolate(d[:, None], size=tuple(frames.shape[-2:]), mode='bilinear', align_corners=True)[:, 0]
        out = {'depth': up(self.depths[first:first + n]), 'carry': {'index': first + n}}
        if pred_bidir_depth:
            out['depth_bwd'] = up(self.depths[first + 1:first + n + 1])
        return out


@pytest.mark.parametrize('mode', ['default', 'sequence'])
@pytest.mark.parametrize('bidir', [False, True])
def test_run_depth_geometry_outputs(tmp_path, mode, bidir):
    pytest.importorskip('PIL')
    from unimatch_amd import depth
    depths = write_plane_scene(tmp_path / 'scene')
    imgs, poses, k = depth.read_scene(str(tmp_path / 'scene'))
    common = dict(padding_factor=8, pred_bidir_depth=bidir, device='cpu', pairs_per_launch=2 if mode == 'sequence' else None)
    stems = [f'{20 * i:04d}' for i in range(T)]
    today = sorted(s + e for s in stems[:-1] for e in (['.png', '_bwd.png'] if bidir else ['.png']))
    depth.run_depth(DepthStandIn(depths, poses), str(tmp_path / 'scene'), str(tmp_path / 'plain'), {}, **common)
    assert sorted(os.listdir(tmp_path / 'plain')) == today                              # without the new flags: today's file set
    ply = str(tmp_path / 'cloud.ply')
    depth.run_depth(DepthStandIn(depths, poses), str(tmp_path / 'scene'), str(tmp_path / 'out'), {}, save_depth=True,
                    consistency_check=True, save_ply=ply, ply_stride=1, **common)
    with_depth = stems if bidir else stems[:-1]                                          # the last frame: only through depth_bwd
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(today + [s + e for s in with_depth for e in ('_depth.png', '_occ.png')])
    for name in today:
        assert np.array_equal(read_png(str(tmp_path / 'out' / name)), read_png(str(tmp_path / 'plain' / name)))
    zeros = 0
    for i, stem in enumerate(with_depth):
        mm = io.read_png16(str(tmp_path / 'out' / (stem + '_depth.png')))
        assert mm.shape == (H, W) and np.abs(mm / 1000. - depths[i].numpy()).max() <= 0.06 * depths[i].max() + 1e-3
        occ = read_png(str(tmp_path / 'out' / (stem + '_occ.png')))
        assert occ.shape == (H, W) and set(np.unique(occ)) <= {0, 255}
        zeros += int((occ == 0).sum())
    xyz, rgb = io.read_ply(ply)
    assert xyz.shape[0] == rgb.shape[0] == zeros and 0.2 * len(with_depth) * H * W < zeros < len(with_depth) * H * W
    if mode == 'default':                              # this mode has no resize round trip: the masks are those of the library call
        from unimatch_amd.video import read_frame_u8
        stand = DepthStandIn(depths, poses)
        pred = torch.stack([stand._depth(i, read_frame_u8(imgs[i])) for i in range(len(with_depth))], 0)
        want = geometry.fuse_depth_sequence(pred, torch.from_numpy(k)[None], torch.from_numpy(poses[:len(with_depth)]))
        for i, stem in enumerate(with_depth):
            assert np.array_equal(read_png(str(tmp_path / 'out' / (stem + '_occ.png'))) == 0, want['keep'][i].numpy() == 1)
        assert np.array_equal(xyz, want['xyz'].numpy())
        red = read_frame_u8(imgs[0])[..., 0] > 200                                       # five percent off: mostly inconsistent
        assert want['keep'][0][red].mean() < 0.2 < want['keep'][0][~red].mean()
    # a larger stride thins the cloud only; the thresholds reach the check
    depth.run_depth(DepthStandIn(depths, poses), str(tmp_path / 'scene'), str(tmp_path / 'out3'), {}, save_ply=ply, ply_stride=3, rel_thr=0.2,
                    **common)
    assert sorted(os.listdir(tmp_path / 'out3')) == today
    loose = io.read_ply(ply)[0].shape[0]
    assert 0 < loose < zeros


def test_run_depth_geometry_errors_and_parser(tmp_path):
    pytest.importorskip('PIL')
    from unimatch_amd import depth, stereo
    depths = write_plane_scene(tmp_path / 'scene')
    _, poses, _ = depth.read_scene(str(tmp_path / 'scene'))
    for name in ('0040', '0060'):                                                        # two frames left: one depth map without bidir
        for sub, ext in (('color', '.png'), ('pose', '.txt')):
            os.remove(tmp_path / 'scene' / sub / (name + ext))
    with pytest.raises(ValueError, match='two frames'):
        depth.run_depth(DepthStandIn(depths, poses), str(tmp_path / 'scene'), str(tmp_path / 'o'), {}, device='cpu', consistency_check=True)
    depth.run_depth(DepthStandIn(depths, poses), str(tmp_path / 'scene'), str(tmp_path / 'o2'), {}, device='cpu', consistency_check=True,
                    pred_bidir_depth=True)
    assert sorted(os.listdir(tmp_path / 'o2')) == ['0000.png', '0000_bwd.png', '0000_occ.png', '0020_occ.png']
    for mod, argv in ((depth, ['--scene', 'x', '--out', 'y', '--ply-stride', 'many']), (stereo, ['--out', 'y', '--lr-check', 'yes'])):
        with pytest.raises(SystemExit) as exc:
            mod.main(argv)
        assert exc.value.code == 2
