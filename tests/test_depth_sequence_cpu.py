"""CPU tests of posed-video depth: ``UniMatch.forward_sequence(task='depth')`` with the CPU oracle injected as hot-path backend
(pairs against the pairwise forward, chunks with a carry, stale carries, how many images the encoder sees, per-frame intrinsics, the
error table), the C ABI of ``um_relative_pose_pairs`` without a GPU, and the sequence mode of the depth runner with a stand-in model."""
import ctypes
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, prepost, visualize
from unimatch_amd.prepost import InferenceGeometry
from unimatch_amd.synth import CONFIGS, synth_camera, synth_frames, synth_state_dict
from tests.oracle_ops import OracleOps
from tests.test_stereo_depth_inference_cpu import read_png, write_frames
from tests.test_video_cpu import EncoderCount, close

T, H, W = 5, 48, 64
NAMES = ['gmdepth_s1', 'gmdepth_s1_rr1']
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _model(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    return model, {k: v for k, v in fk.items() if k != 'task'}


def scene(frames=T, h=H, w=W, seed=2100):
    """Normalised frames ``[T, 3, h, w]``, intrinsics ``[1, 3, 3]`` and absolute poses ``[T, 4, 4]``: ``synth_camera``'s relative pose
    is ``inv(P[t + 1]) @ P[t]`` of every pair, so ``P[t + 1] = P[t] @ inv(rel)`` from ``P[0] = I`` (in float64, rounded once)."""
    x = synth_frames(frames, h, w, seed=seed) / 255.
    x = ((x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).contiguous()
    k, rel = synth_camera(1, h, w)
    step = torch.linalg.inv(rel[0].double())
    poses = [torch.eye(4, dtype=torch.float64)]
    for _ in range(frames - 1):
        poses.append(poses[-1] @ step)
    return x, k, torch.stack(poses, 0).float()


def host_relative(poses):
    """The pairwise protocol's pose: ``inv(pose_tgt) @ pose_ref`` in fp32 (evaluate_depth.py:347-350)."""
    return torch.linalg.inv(poses[1:]) @ poses[:-1]


def pairwise(model, kw, x, k, poses, bidir=False, **more):
    """``model(f[i], f[i + 1], task='depth', ...)`` of every pair -> ``(forward [T-1, H, W], backward or None)``."""
    rel = host_relative(poses)
    kk = k.expand(x.shape[0], 3, 3)
    outs = [model(x[i:i + 1], x[i + 1:i + 2], task='depth', intrinsics=kk[i:i + 1], pose=rel[i:i + 1], pred_bidir_depth=bidir,
                  **dict(kw, **more))['flow_preds'][0] for i in range(x.shape[0] - 1)]
    fwd = torch.cat([o[:1] for o in outs], 0)
    return fwd, (torch.cat([o[1:] for o in outs], 0) if bidir else None)


@pytest.fixture(scope='module', params=NAMES)
def seq(request):
    model, kw = _model(request.param)
    x, k, poses = scene()
    return model, kw, x, k, poses, pairwise(model, kw, x, k, poses, bidir=True)


# ------------------------------------------------------------------ 1. sequence equals pairwise
@pytest.mark.parametrize('step', [8, 2, 1])
def test_sequence_matches_pairwise(seq, step):
    model, kw, x, k, poses, (fwd, bwd) = seq
    out = model.forward_sequence(x, task='depth', intrinsics=k, poses=poses, pairs_per_launch=step, **kw)
    assert set(out) == {'depth', 'carry'} and tuple(out['depth'].shape) == (T - 1, H, W)
    assert close(out['depth'], fwd), step
    out = model.forward_sequence(x, task='depth', intrinsics=k, poses=poses, pairs_per_launch=step, pred_bidir_depth=True, colorize=True,
                                 **kw)
    assert set(out) == {'depth', 'depth_bwd', 'depth_rgb', 'depth_bwd_rgb', 'carry'}
    assert tuple(out['depth'].shape) == tuple(out['depth_bwd'].shape) == (T - 1, H, W)
    assert tuple(out['depth_rgb'].shape) == tuple(out['depth_bwd_rgb'].shape) == (T - 1, H, W, 3) and out['depth_rgb'].dtype == torch.uint8
    assert close(out['depth'], fwd) and close(out['depth_bwd'], bwd), step
    assert torch.equal(out['depth_rgb'], visualize.inverse_depth_to_image(out['depth']))
    assert torch.equal(out['depth_bwd_rgb'], visualize.inverse_depth_to_image(out['depth_bwd']))
    assert set(out['carry']) == {'features', 'frame', 'state', 'pose', 'intrinsics'}
    assert torch.equal(out['carry']['pose'], poses[-1:]) and torch.equal(out['carry']['intrinsics'], k)


def test_depth_from_argmax_shape_and_finiteness(seq):
    """An argmax may flip on rounding noise between batch sizes: shape and finiteness only."""
    model, kw, x, k, poses, _ = seq
    out = model.forward_sequence(x, task='depth', intrinsics=k, poses=poses, pairs_per_launch=2, depth_from_argmax=True,
                                 pred_bidir_depth=True, **kw)
    assert set(out) == {'depth', 'depth_bwd', 'carry'}
    for key in ('depth', 'depth_bwd'):
        assert tuple(out[key].shape) == (T - 1, H, W) and torch.isfinite(out[key]).all()
        assert (out[key] >= 1 / kw['max_depth'] - 1e-6).all() and (out[key] <= 1 / kw['min_depth'] + 1e-5).all()


# ------------------------------------------------------------------ 2. the encoder sees T images, against 2 (T - 1)
def test_encoder_sees_each_frame_once(seq):
    model, kw, x, k, poses, _ = seq
    count = EncoderCount(model)
    try:
        model.forward_sequence(x, task='depth', intrinsics=k, poses=poses, pairs_per_launch=2, **kw)
        assert count.images == T
        count.images = 0
        pairwise(model, kw, x, k, poses)
        assert count.images == 2 * (T - 1)
    finally:
        del model.backbone.forward


# ------------------------------------------------------------------ 3. the carry
def test_pieces_with_carry_equal_one_call(seq):
    model, kw, x, k, poses, _ = seq
    args = dict(task='depth', intrinsics=k, pred_bidir_depth=True, colorize=True, **kw)
    keys = ('depth', 'depth_bwd', 'depth_rgb', 'depth_bwd_rgb')
    # chunks of two pairs from frame 0 and from frame 3: the chunk shapes of the one call -> bitwise
    whole = model.forward_sequence(x, poses=poses, pairs_per_launch=2, **args)
    count = EncoderCount(model)
    try:
        a = model.forward_sequence(x[:3], poses=poses[:3], pairs_per_launch=2, **args)
        b = model.forward_sequence(x[3:], poses=poses[3:], pairs_per_launch=2, carry=a['carry'], **args)
    finally:
        del model.backbone.forward
    assert count.images == T                                          # the carried frame is not encoded again
    assert a['depth'].shape[0] == 2 and b['depth'].shape[0] == 2
    for key in keys:
        assert torch.equal(torch.cat([a[key], b[key]], 0), whole[key]), key
    assert torch.equal(b['carry']['pose'], whole['carry']['pose']) and torch.equal(b['carry']['frame'], whole['carry']['frame'])
    # other chunk shapes (3 + 1 pairs against 4): within the file's tolerance, the colours not compared
    whole = model.forward_sequence(x, poses=poses, pairs_per_launch=8, **args)
    a = model.forward_sequence(x[:4], poses=poses[:4], pairs_per_launch=8, **args)
    b = model.forward_sequence(x[4:], poses=poses[4:], pairs_per_launch=8, carry=a['carry'], **args)
    assert a['depth'].shape[0] == 3 and b['depth'].shape[0] == 1
    for key in keys[:2]:
        assert close(torch.cat([a[key], b[key]], 0), whole[key]), key


def test_stale_carry_is_encoded_again():
    model, kw = _model('gmdepth_s1')
    x, k, poses = scene(seed=2101)
    args = dict(task='depth', intrinsics=k, **kw)
    a = model.forward_sequence(x[:3], poses=poses[:3], **args)
    with torch.no_grad():
        model.backbone.conv1.weight.mul_(0.5)                         # in-place edit: the carry's features are stale
    count = EncoderCount(model)
    try:
        b = model.forward_sequence(x[3:], poses=poses[3:], carry=a['carry'], **args)
    finally:
        del model.backbone.forward
    assert count.images == T - 3 + 1                                  # the carried frame went through the encoder again
    fresh = model.forward_sequence(x[2:], poses=poses[2:], **args)
    assert torch.equal(b['depth'], fresh['depth'])                    # with the carried pose and intrinsics
    # a flow carry holds no pose, a depth carry holds features of normalised frames: neither crosses over
    flow_ck, flow_kw = CONFIGS['gmflow_s1']
    flow = UniMatch(**flow_ck).eval().bind_ops(OracleOps())
    flow_kw = {key: v for key, v in flow_kw.items() if key != 'task'}
    with pytest.raises(ValueError):
        flow.forward_sequence(x[3:], carry=a['carry'], **flow_kw)
    flow_carry = flow.forward_sequence(synth_frames(2, H, W), **flow_kw)['carry']
    with pytest.raises(ValueError):
        model.forward_sequence(x[3:], poses=poses[3:], carry=flow_carry, **args)
    with pytest.raises(ValueError):                                   # a carry of another geometry
        model.forward_sequence(scene(2, 32, 64)[0], poses=poses[3:], carry=b['carry'], **args)


def test_the_joining_pair_uses_the_carried_pose_and_intrinsics(seq):
    """The pair that joins two pieces is (carried frame, first new frame): its reference pose and its intrinsics row are the carry's.
    The pose of the first new frame is that pair's TARGET pose (``rel = inv(poses[t + 1]) @ poses[t]``), so changing it moves the
    joining pair and the one after it and nothing else; what must not reach the joining pair is the first new frame's intrinsics row
    (pair t uses row t), and what must reach it is a change of the carried pose."""
    model, kw, x, k, poses, _ = seq
    kt = k.repeat(T, 1, 1)
    args = dict(task='depth', pairs_per_launch=8, **kw)
    whole = model.forward_sequence(x, intrinsics=kt, poses=poses, **args)['depth']
    a = model.forward_sequence(x[:2], intrinsics=kt[:2], poses=poses[:2], **args)
    b = model.forward_sequence(x[2:], intrinsics=kt[2:], poses=poses[2:], carry=a['carry'], **args)['depth']     # pairs 1, 2, 3
    assert close(b, whole[1:])
    # the first new frame's intrinsics row belongs to the pair after the joining one
    k2 = kt[2:].clone()
    k2[0, 0, 0] *= 1.2
    moved = model.forward_sequence(x[2:], intrinsics=k2, poses=poses[2:], carry=a['carry'], **args)['depth']
    assert torch.equal(moved[0], b[0]) and not torch.equal(moved[1], b[1]) and torch.equal(moved[2], b[2])
    # the carried pose is the joining pair's reference pose and nobody else's
    carry = dict(a['carry'])
    carry['pose'] = carry['pose'].clone()
    carry['pose'][0, 0, 3] += 0.3
    moved = model.forward_sequence(x[2:], intrinsics=kt[2:], poses=poses[2:], carry=carry, **args)['depth']
    assert not torch.equal(moved[0], b[0]) and torch.equal(moved[1:], b[1:])
    # the first new frame's pose: target of the joining pair, reference of the next
    p2 = poses[2:].clone()
    p2[0, 0, 3] += 0.3
    moved = model.forward_sequence(x[2:], intrinsics=kt[2:], poses=p2, carry=a['carry'], **args)['depth']
    assert not torch.equal(moved[0], b[0]) and not torch.equal(moved[1], b[1]) and torch.equal(moved[2], b[2])
    # a joining pair whose reference pose were poses[0] of the second piece would have the identity as relative pose
    rel = host_relative(poses[1:3])
    want = model(x[1:2], x[2:3], task='depth', intrinsics=k, pose=rel, **kw)['flow_preds'][0]
    same = model(x[1:2], x[2:3], task='depth', intrinsics=k, pose=torch.eye(4)[None], **kw)['flow_preds'][0]
    assert close(b[:1], want) and not close(b[:1], same)


# ------------------------------------------------------------------ 4. per-frame intrinsics
def test_per_frame_intrinsics_reach_only_their_pair(seq):
    model, kw, x, k, poses, (fwd, _) = seq
    args = dict(task='depth', poses=poses, pairs_per_launch=8, **kw)
    kt = k.repeat(T, 1, 1)
    base = model.forward_sequence(x, intrinsics=kt, **args)['depth']
    assert torch.equal(base, model.forward_sequence(x, intrinsics=k, **args)['depth'])
    k2 = kt.clone()
    k2[2, 0, 0] *= 1.2
    k2[2, 1, 2] += 3.0
    got = model.forward_sequence(x, intrinsics=k2, **args)['depth']
    for i in range(T - 1):
        assert torch.equal(got[i], base[i]) == (i != 2), i
    want = pairwise(model, kw, x, k2, poses)[0]                       # pair 2 with row 2 for both views
    assert close(got, want) and not close(got[2:3], fwd[2:3])
    k3 = kt.clone()
    k3[T - 1, 0, 0] *= 1.2                                            # the last frame starts no pair of this call ...
    out = model.forward_sequence(x, intrinsics=k3, **args)
    assert torch.equal(out['depth'], base) and torch.equal(out['carry']['intrinsics'], k3[T - 1:])   # ... it is carried


# ------------------------------------------------------------------ 5. errors
def test_error_table(seq):
    model, kw, x, k, poses, _ = seq
    args = dict(task='depth', intrinsics=k, poses=poses, **kw)
    with pytest.raises(NotImplementedError, match='share no frame'):
        model.forward_sequence(x, **dict(args, task='stereo'))
    for bad in (dict(poses=None), dict(intrinsics=None), dict(poses=poses[:T - 1]), dict(poses=poses[0]), dict(intrinsics=k.repeat(2, 1, 1)),
                dict(intrinsics=k[0]), dict(intrinsics=k.repeat(T + 1, 1, 1)), dict(pairs_per_launch=0)):
        with pytest.raises(ValueError):
            model.forward_sequence(x, **dict(args, **bad))
    with pytest.raises(ValueError):
        model.forward_sequence(x[:1], **dict(args, poses=poses[:1]))
    for bad in (dict(pred_bidir_flow=True), dict(consistency_check=True), dict(pred_bidir_flow=True, consistency_check=True)):
        with pytest.raises(AssertionError):
            model.forward_sequence(x, **dict(args, **bad))
    ck, fk = CONFIGS['gmflow_s2_rr6']
    two = UniMatch(**ck).eval().bind_ops(OracleOps())
    assert two.num_scales != 1
    with pytest.raises(AssertionError):
        two.forward_sequence(x, task='depth', intrinsics=k, poses=poses, attn_type='swin', attn_splits_list=[2, 8],
                             prop_radius_list=[-1, 1])
    with pytest.raises(AssertionError):                               # forward raises the same
        two(x[:1], x[1:2], task='depth', intrinsics=k, pose=host_relative(poses[:2]), attn_type='swin', attn_splits_list=[2, 8],
            prop_radius_list=[-1, 1])


def test_flow_ignores_the_depth_keywords():
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    kw = {k: v for k, v in fk.items() if k != 'task'}
    frames = synth_frames(3, H, W, seed=2102)
    plain = model.forward_sequence(frames, **kw)
    other = model.forward_sequence(frames, intrinsics=torch.zeros(7, 3, 3), poses=torch.zeros(9, 4, 4), min_depth=3., max_depth=4.,
                                   num_depth_candidates=5, depth_from_argmax=True, pred_bidir_depth=True, **kw)
    assert set(other) == set(plain) == {'flow', 'carry'} and torch.equal(other['flow'], plain['flow'])
    assert set(plain['carry']) == {'features', 'frame', 'state'}


# ------------------------------------------------------------------ 6. C ABI without a GPU
def test_relative_pose_symbol_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'unimatch_hip.h')).read()
    name = 'um_relative_pose_pairs'
    assert f'int {name}(const float* poses, float* rel, int frames, void* stream);' in text
    assert hasattr(lib, name) and name in _abi.SIGNATURES
    res, args = _abi.SIGNATURES[name]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    from unimatch_amd.ops import HipOps
    assert callable(HipOps.relative_pose_pairs)


def test_relative_pose_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(16)
    assert lib.um_relative_pose_pairs(None, p, 4, None) == -1
    assert b'um_relative_pose_pairs' in lib.um_last_error_string()
    assert lib.um_relative_pose_pairs(p, None, 4, None) == -1
    assert lib.um_relative_pose_pairs(p, p, 1, None) == -1
    assert lib.um_relative_pose_pairs(p, p, 0, None) == -1
    assert lib.um_relative_pose_pairs(p, p, -3, None) == -1


# ------------------------------------------------------------------ 7. the runner's sequence mode, with a stand-in model
class SequenceStandIn:
    """Stands in for the model in ``run_depth(pairs_per_launch=N)``: a deterministic ``forward_sequence`` whose "depth" of pair t is
    a smooth function of the two prepared frames, with a carry that holds the last frame."""

    def __init__(self):
        self.calls, self.frames, self.poses = [], [], []

    @staticmethod
    def _value(a, b):
        return (a[:, 0] - 0.5 * b[:, 1]).abs() + 0.05 * a[:, 2].abs() + 0.5

    def predict(self, *a, **k):
        raise AssertionError('sequence mode does not call predict')

    def forward_sequence(self, frames, carry=None, poses=None, pred_bidir_depth=False, **kw):
        self.calls.append(dict(kw, pred_bidir_depth=pred_bidir_depth, count=frames.shape[0], size=tuple(frames.shape[2:]),
                               carried=carry is not None))
        self.frames.extend(frames)
        self.poses.extend(poses)
        assert poses.shape[0] == frames.shape[0]
        x = frames if carry is None else torch.cat([carry['frame'], frames], 0)
        out = {'depth': self._value(x[:-1], x[1:]), 'carry': {'frame': x[-1:].clone()}}
        if pred_bidir_depth:
            out['depth_bwd'] = self._value(x[1:], x[:-1])
        return out


def write_scene(root, names, h, w, seed=8):
    images = write_frames(str(root / 'color'), names, h, w, seed=seed)
    (root / 'pose').mkdir()
    (root / 'intrinsic').mkdir()
    rng = np.random.default_rng(seed + 1)
    for i, name in enumerate(names):
        ang = 0.03 * i
        p = np.eye(4)
        p[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        p[:3, 3] = rng.standard_normal(3) * 0.1
        np.savetxt(str(root / 'pose' / name.replace('.png', '.txt')), p, delimiter=' ')
    k4 = np.eye(4)
    k4[:3, :3] = [[577.59, 0, 20.1], [0, 578.73, 12.2], [0, 0, 1]]
    np.savetxt(str(root / 'intrinsic' / 'intrinsic_depth.txt'), k4)
    return images


@pytest.mark.parametrize('bidir', [False, True])
@pytest.mark.parametrize('step', [1, 2, 8])
def test_run_depth_sequence_mode_writes_the_default_modes_file_set(tmp_path, bidir, step):
    pytest.importorskip('PIL')
    from unimatch_amd import depth
    from tests.test_stereo_depth_inference_cpu import StandIn
    h, w = 24, 40
    names = [f'{i:04d}.png' for i in (0, 20, 40, 60)]
    images = write_scene(tmp_path / 'scene', names, h, w)
    imgs, poses, k = depth.read_scene(str(tmp_path / 'scene'))
    fwd_kw = {'attn_type': 'swin', 'task': 'depth', 'min_depth': 0.1, 'max_depth': 2.0}
    common = dict(padding_factor=16, min_depth=0.5, max_depth=10., num_depth_candidates=32, pred_bidir_depth=bidir, device='cpu')
    assert depth.run_depth(StandIn(), str(tmp_path / 'scene'), str(tmp_path / 'default'), fwd_kw, **common) == 3
    model = SequenceStandIn()
    out = tmp_path / 'out'
    assert depth.run_depth(model, str(tmp_path / 'scene'), str(out), fwd_kw, pairs_per_launch=step, **common) == 3
    assert sorted(os.listdir(out)) == sorted(os.listdir(tmp_path / 'default'))
    assert sorted(os.listdir(out)) == sorted(s + e for s in ('0000', '0020', '0040') for e in (['.png', '_bwd.png'] if bidir else ['.png']))
    # pieces of at most step + 1 frames joined by the carry; every frame once, prepared at (32, 48); the absolute poses as read
    assert [c['count'] for c in model.calls] == {1: [2, 1, 1], 2: [3, 1], 8: [4]}[step]
    assert [c['carried'] for c in model.calls] == [False] + [True] * (len(model.calls) - 1)
    geom = InferenceGeometry.resized((h, w), (32, 48))
    prepared = geom.prepare(torch.from_numpy(np.stack(images, 0)), normalize=True)[0]
    assert len(model.frames) == 4 and torch.equal(torch.stack(model.frames, 0), prepared)
    assert torch.stack(model.poses, 0).dtype == torch.float32 and np.array_equal(torch.stack(model.poses, 0).numpy(), poses)
    for c in model.calls:
        assert c['task'] == 'depth' and c['size'] == (32, 48) and c['attn_type'] == 'swin' and c['pairs_per_launch'] == step
        assert c['min_depth'] == 1 / 10. and c['max_depth'] == 1 / 0.5 and c['num_depth_candidates'] == 32
        assert c['pred_bidir_depth'] == bidir and c['depth_from_argmax'] is False
        assert torch.equal(c['intrinsics'], torch.from_numpy(k)[None])                       # not rescaled, as in the reference
    fwd = geom.restore(SequenceStandIn._value(prepared[:-1], prepared[1:]), 'depth')
    bwd = geom.restore(SequenceStandIn._value(prepared[1:], prepared[:-1]), 'depth')
    for i, stem in enumerate(('0000', '0020', '0040')):
        assert np.array_equal(read_png(str(out / (stem + '.png'))), visualize.inverse_depth_to_image(fwd[i:i + 1])[0].numpy())
        if bidir:
            assert np.array_equal(read_png(str(out / (stem + '_bwd.png'))), visualize.inverse_depth_to_image(bwd[i:i + 1])[0].numpy())


def test_run_depth_sequence_mode_intrinsics_scaling_sizes_and_parser(tmp_path):
    pytest.importorskip('PIL')
    from unimatch_amd import depth, io
    h, w = 24, 40
    names = [f'{i:04d}.png' for i in range(4)]
    write_scene(tmp_path / 'scene', names, h, w)
    _, _, k = depth.read_scene(str(tmp_path / 'scene'))
    model = SequenceStandIn()
    depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'out'), {}, padding_factor=16, scale_intrinsics=True, device='cpu',
                    pairs_per_launch=2)
    want_k = InferenceGeometry.resized((h, w), (32, 48)).scaled_intrinsics(torch.from_numpy(k)[None])
    assert all(torch.equal(c['intrinsics'], want_k) for c in model.calls) and not torch.equal(want_k, torch.from_numpy(k)[None])
    model = SequenceStandIn()
    depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'out'), {}, inference_size=(16, 64), device='cpu', pairs_per_launch=2)
    assert all(c['size'] == (16, 64) for c in model.calls)
    with pytest.raises(ValueError):
        depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'out'), {}, device='cpu', pairs_per_launch=0)
    # a frame of another size: refused by name (the default mode takes it: every pair has its own geometry there)
    io.write_png8(str(tmp_path / 'scene' / 'color' / '0002.png'), np.zeros((h + 8, w, 3), np.uint8))
    with pytest.raises(ValueError, match='0002.png'):
        depth.run_depth(SequenceStandIn(), str(tmp_path / 'scene'), str(tmp_path / 'out2'), {}, device='cpu', pairs_per_launch=8)
    ap_error = None
    try:
        depth.main(['--scene', 'x', '--out', 'y', '--pairs-per-launch', 'many'])
    except SystemExit as exc:
        ap_error = exc.code
    assert ap_error == 2
