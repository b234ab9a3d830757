"""GPU tests of posed-video depth: ``um_relative_pose_pairs`` against an fp64 evaluation of ``inv(P[t + 1]) @ P[t]``, and
``UniMatch.forward_sequence(task='depth')`` (each frame encoded once, relative poses on the device, no synchronisation) against the
pairwise forward with the host's fp32 relative pose."""
import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, visualize
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_frames, synth_state_dict
from tests.test_video_gpu import floor_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope='module')
def ops():
    from unimatch_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------ 1. the kernel
def random_poses(count, seed):
    """``[count, 4, 4]`` fp32: axis-angle rotations up to pi, translations within +-5; every third pose has its rotation block scaled
    per axis (affine, not orthonormal: the general inverse)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, 4, 4))
    for i in range(count):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0, np.pi)
        kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        rot = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        if i % 3 == 1:
            rot = rot @ np.diag(rng.uniform(0.5, 2.0, 3))
        out[i, :3, :3] = rot
        out[i, :3, 3] = rng.uniform(-5, 5, 3)
        out[i, 3, 3] = 1
    return torch.from_numpy(out.astype(np.float32))


def relative_fp64(poses):
    p = poses.double().numpy()
    return torch.from_numpy(np.linalg.inv(p[1:]) @ p[:-1])


@pytest.mark.parametrize('count', [2, 7, 130])
def test_relative_pose_pairs_against_fp64(ops, count):
    poses = random_poses(count, seed=count)
    want = relative_fp64(poses)
    got = ops.relative_pose_pairs(poses.to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (count - 1, 4, 4)
    got = got.cpu()
    bound = 2e-6 * want.abs().max().item()
    worst = (got.double() - want).abs().max().item()
    print(f'relative_pose_pairs T={count}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst < bound
    bottom = torch.tensor([0., 0., 0., 1.]).expand(count - 1, 4)
    assert torch.equal(got[:, 3], bottom)
    assert torch.equal(ops.relative_pose_pairs(poses.to(DEV)).cpu(), got)
    # chained through the camera packing: the bound of um_depth_cam_pack against the packing of the true relative poses
    k = synth_camera(count - 1, 240, 320)[0]
    kd = k.double().clone()
    kd[:, :2] /= 8.0
    for bidir in (False, True):
        cam = ops.depth_cam(k.to(DEV), ops.relative_pose_pairs(poses.to(DEV)), 8.0, bidir).cpu().double()
        pd = torch.cat([want, torch.linalg.inv(want)], 0) if bidir else want
        kk = kd.repeat(2, 1, 1) if bidir else kd
        packed = torch.cat([torch.linalg.inv(kk).flatten(1), pd[:, :3, :3].flatten(1), pd[:, :3, 3], kk.flatten(1)], 1)
        worst = (cam - packed).abs().max().item()
        print(f'  depth_cam bidir={bidir}: max error {worst:.3e}, bound {2e-6 * packed.abs().max().item():.3e}')
        assert cam.shape == packed.shape and worst < 2e-6 * packed.abs().max().item()
    if count < 3:
        return
    # frame s singular (a zero row: the fp64 determinant is exactly 0): pair s - 1, which inverts it, is NaN in its upper rows; pair s
    # reads it as its reference pose and stays finite; nobody else sees it
    s = count // 2
    sing = poses.clone()
    sing[s, 2, :3] = 0.0
    bad = ops.relative_pose_pairs(sing.to(DEV)).cpu()
    assert torch.isnan(bad[s - 1, :3]).all() and torch.equal(bad[s - 1, 3], bottom[0])
    keep = [t for t in range(count - 1) if t not in (s - 1, s)]
    assert torch.equal(bad[keep], got[keep]) and torch.isfinite(bad[keep]).all() and torch.isfinite(bad[s]).all()


def test_relative_pose_pairs_refuses_bad_arguments(ops):
    with pytest.raises(ValueError):
        ops.relative_pose_pairs(torch.eye(4, device=DEV)[None])
    with pytest.raises(ValueError):
        ops.relative_pose_pairs(torch.zeros(3, 3, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.relative_pose_pairs(torch.eye(4)[None].repeat(3, 1, 1))


# ------------------------------------------------------------------ 2. the sequence against the pairwise forward
def _model(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    return model.to(DEV), {k: v for k, v in fk.items() if k != 'task'}


def scene(frames, h, w, seed):
    """Normalised frames, intrinsics ``[1, 3, 3]`` and absolute poses whose consecutive relative pose is ``synth_camera``'s."""
    x = synth_frames(frames, h, w, seed=seed) / 255.
    x = ((x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).contiguous()
    k, rel = synth_camera(1, h, w)
    step = torch.linalg.inv(rel[0].double())
    poses = [torch.eye(4, dtype=torch.float64)]
    for _ in range(frames - 1):
        poses.append(poses[-1] @ step)
    return x.to(DEV), k.to(DEV), torch.stack(poses, 0).float()


def host_relative(poses):
    """``inv(pose_tgt) @ pose_ref`` in fp32 on the host (``depth.relative_pose``)."""
    p = poses.numpy().astype(np.float32)
    return torch.from_numpy((np.linalg.inv(p[1:]) @ p[:-1]).astype(np.float32))


@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_sequence_against_pairwise(name):
    model, kw = _model(name)
    T, H, W = 6, 96, 128
    x, k, poses = scene(T, H, W, seed=177)
    rel = host_relative(poses).to(DEV)
    poses = poses.to(DEV)
    pairwise = torch.stack([model(x[i:i + 1], x[i + 1:i + 2], task='depth', intrinsics=k, pose=rel[i:i + 1], pred_bidir_depth=True,
                                  **kw)['flow_preds'][0] for i in range(T - 1)], 0)               # [T - 1, 2, H, W]
    calls = [0]
    inner = model.backbone.forward

    def counted(x, *a, **kws):
        calls[0] += (x.shape[0] if torch.is_tensor(x) else sum(t.shape[0] for t in x))
        return inner(x, *a, **kws)
    model.backbone.forward = counted
    args = dict(task='depth', intrinsics=k, pairs_per_launch=3, pred_bidir_depth=True, colorize=True, **kw)
    try:
        out = model.forward_sequence(x, poses=poses, **args)
    finally:
        del model.backbone.forward
    assert calls[0] == T
    keys = ('depth', 'depth_bwd', 'depth_rgb', 'depth_bwd_rgb')
    assert set(out) == set(keys) | {'carry'}
    assert tuple(out['depth'].shape) == tuple(out['depth_bwd'].shape) == (T - 1, H, W)
    assert torch.isfinite(out['depth']).all() and torch.isfinite(out['depth_bwd']).all()
    for i in range(T - 1):
        for key, want in (('depth', pairwise[i, 0]), ('depth_bwd', pairwise[i, 1])):
            d = (out[key][i] - want).abs().max().item()
            print(f'{name} pair {i} {key}: max |diff| {d:.3e}, floor {1e-3 * max(1.0, want.abs().max().item()):.3e}')
    for i in range(T - 1):
        assert floor_close(out['depth'][i], pairwise[i, 0]), i
        assert floor_close(out['depth_bwd'][i], pairwise[i, 1]), i
    again = model.forward_sequence(x, poses=poses, **args)
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(again[key], out[key]), key
    assert torch.equal(visualize.inverse_depth_to_image(out['depth']), out['depth_rgb'])
    assert torch.equal(visualize.inverse_depth_to_image(out['depth_bwd']), out['depth_bwd_rgb'])
    assert out['depth_rgb'].dtype == torch.uint8 and tuple(out['depth_rgb'].shape) == (T - 1, H, W, 3)
    # fed in pieces with the carry: chunks of 3 + 2 pairs from frame 0, and 3 from frame 0 + 2 behind the carry -> the same chunk shapes
    a = model.forward_sequence(x[:4], poses=poses[:4], **args)
    b = model.forward_sequence(x[4:], poses=poses[4:], carry=a['carry'], **args)
    for key in keys:
        assert torch.equal(torch.cat([a[key], b[key]], 0), out[key]), key
    model.check_operand_range()


# ------------------------------------------------------------------ 3. no synchronisation
def test_depth_sequence_never_synchronises():
    model, kw = _model('gmdepth_s1_rr1')
    x, k, poses = scene(5, 96, 128, seed=178)
    poses = poses.to(DEV)
    args = dict(task='depth', intrinsics=k, poses=poses, pairs_per_launch=2, pred_bidir_depth=True, colorize=True, **kw)
    first = model.forward_sequence(x, **args)                           # library, allocator, weight planes, tables warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                             # the mode does catch a synchronising call
        got = model.forward_sequence(x, **args)
        head = model.forward_sequence(x[:3], **dict(args, poses=poses[:3]))
        piece = model.forward_sequence(x[3:], **dict(args, poses=poses[3:], carry=head['carry']))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    for key in ('depth', 'depth_bwd', 'depth_rgb', 'depth_bwd_rgb'):
        assert torch.equal(got[key], first[key]), key
        assert torch.equal(piece[key], first[key][2:]), key


# ------------------------------------------------------------------ 4. concurrent parts
@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_sequence_parts_are_the_match_step_of_each_half(name):
    model, kw = _model(name)
    T, H, W = 5, 96, 128
    x, k, poses = scene(T, H, W, seed=179)
    kt = k.repeat(T, 1, 1).contiguous()
    kt[:, 0, 0] *= torch.linspace(1.0, 1.1, T, device=DEV)               # per-frame rows: a wrong shard would show
    poses = poses.to(DEV)
    args = dict(task='depth', intrinsics=kt, poses=poses, pairs_per_launch=4, pred_bidir_depth=True, **kw)
    model.launch_parts = 2
    try:
        out = model.forward_sequence(x, **args)                          # first call: the parts one after the other
        runs = [model.forward_sequence(x, **args) for _ in range(2)]     # then on two streams
        torch.cuda.synchronize()
        for r in runs:
            assert torch.equal(r['depth'], out['depth']) and torch.equal(r['depth_bwd'], out['depth_bwd'])
        with torch.no_grad():
            feats = model._encode((x,), 'depth')
            rel = model.ops.relative_pose_pairs(poses)
            kwm = dict(kw, task='depth', pred_bidir_depth=True)
            for lo, hi in ((0, 2), (2, 4)):
                stream = [torch.cat([f[lo:hi], f[lo + 1:hi + 1]], 0) for f in feats]
                part = model._match(stream, hi - lo, intrinsics=kt[lo:hi], pose=rel[lo:hi], **kwm)['flow_preds'][0]
                assert torch.equal(part[:hi - lo], out['depth'][lo:hi]), (lo, hi)
                assert torch.equal(part[hi - lo:], out['depth_bwd'][lo:hi]), (lo, hi)
    finally:
        model.launch_parts = None
    model.check_operand_range()
