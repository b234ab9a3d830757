"""CPU tests of the depth confidence (``unimatch_amd.confidence``, the plane sweep's distribution): the host restatement against the
``match_prob`` the reference returns in float64 (tests/golden/depth_stats.npz), the identities of the statistics, the C ABI's argument
checks without a GPU, ``UniMatch.forward_with_depth_confidence`` and ``forward_sequence(task='depth', return_confidence=True)`` with
the CPU oracle injected as hot-path backend, and the confidence filter of ``geometry.fuse_depth_sequence``."""
import math
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, confidence, geometry
from unimatch_amd.synth import CONFIGS, synth_camera, synth_frames, synth_state_dict
from tests.oracle_ops import OracleOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depth_stats.npz')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FLOATS = ('max_prob', 'entropy', 'variance', 'peak_mass')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _tokens(m):
    """``[B, C, h, w]`` -> token-major ``[B, h*w, C]`` float64."""
    t = torch.from_numpy(np.asarray(m, dtype=np.float64))
    return t.flatten(2).transpose(1, 2).contiguous()


def _cam(k, pose):
    return torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous()


def _case(golden, move, bidir):
    """Token features, the packed camera record and the reference's results of one golden case, all float64."""
    f0, f1 = _tokens(golden[f'{move}_f0']), _tokens(golden[f'{move}_f1'])
    k, pose = torch.from_numpy(golden[f'{move}_intrinsics']), torch.from_numpy(golden[f'{move}_pose'])
    if bidir:                                                              # the caller's concatenation, as in the model
        f0, f1 = torch.cat([f0, f1], 0), torch.cat([f1, f0], 0)
        k, pose = k.repeat(2, 1, 1), torch.cat([pose, torch.inverse(pose)], 0)
    tag = '_bidir' if bidir else ''
    ref = {key: torch.from_numpy(golden[f'{move}_{key}{tag}']) for key in ('prob', 'depth', 'depth_argmax')}
    h, w = golden[f'{move}_f0'].shape[-2:]
    return f0, f1, h, w, _cam(k, pose), torch.from_numpy(golden['candidates']), ref


@pytest.mark.parametrize('bidir', [False, True])
@pytest.mark.parametrize('move', ['sideways', 'forward'])
def test_host_restatement_reproduces_the_reference_prob(golden, move, bidir):
    """The same arithmetic in float64: ``match_prob`` and both depth read-outs within 1e-10."""
    f0, f1, h, w, cam, cand, ref = _case(golden, move, bidir)
    prob = confidence.depth_match_prob_host(f0, f1, h, w, cam, cand)
    assert prob.dtype == torch.float64 and prob.shape == ref['prob'].shape
    err = (prob - ref['prob']).abs().max().item()
    soft = (prob * cand.view(1, -1, 1, 1)).sum(1, keepdim=True)
    hard = cand[prob.argmax(1, keepdim=True)]
    print(f'{move} bidir={bidir}: prob {err:.3e} soft-argmin {(soft - ref["depth"]).abs().max().item():.3e} '
          f'arg-max {(hard - ref["depth_argmax"]).abs().max().item():.3e}')
    assert err <= 1e-10
    assert (soft - ref['depth']).abs().max().item() <= 1e-10 and (hard - ref['depth_argmax']).abs().max().item() <= 1e-10
    # the fixture spans flat and peaked distributions
    assert ref['prob'].max(1)[0].min() < 0.1 and ref['prob'].max(1)[0].max() > 0.3


@pytest.mark.parametrize('move', ['sideways', 'forward'])
def test_statistics_of_the_golden_prob_obey_their_identities(golden, move):
    prob, cand = torch.from_numpy(golden[f'{move}_prob_bidir']), torch.from_numpy(golden['candidates'])
    d = prob.shape[1]
    seen = torch.zeros(prob[:, 0].shape, dtype=torch.int32)
    s = confidence.depth_stats_from_prob_host(prob, cand, seen, 1)
    assert bool((s.entropy >= 0).all()) and bool((s.entropy <= math.log(d)).all())
    assert bool((s.max_prob <= s.peak_mass).all()) and bool((s.peak_mass <= 1).all())
    assert bool((s.variance >= 0).all()) and s.variance.max().item() <= (cand.max() - cand.min()).item() ** 2
    whole = confidence.depth_stats_from_prob_host(prob, cand, seen, d)
    assert (whole.peak_mass - 1).abs().max().item() <= 4 * d * torch.finfo(torch.float64).eps
    point = confidence.depth_stats_from_prob_host(prob, cand, seen, 0)
    assert torch.equal(point.peak_mass, point.max_prob) and torch.equal(point.max_prob, s.max_prob)
    assert torch.equal(prob.argmax(1).to(torch.int32), s.best) and s.best.dtype == torch.int32 and s.in_view is seen
    with pytest.raises(ValueError):
        confidence.depth_stats_from_prob_host(prob, cand, seen, -1)


def test_in_view_counts_the_candidates_that_land_in_the_image(golden):
    f0, f1, h, w, cam, cand, _ = _case(golden, 'sideways', False)
    s = confidence.depth_match_stats(f0, f1, h, w, cam, cand)             # host tensors: the host path
    assert s.in_view.dtype == torch.int32 and 0 < s.in_view.min().item() and s.in_view.max().item() == cand.numel()
    away = cam.clone()
    away[:, 18] = 15.0                                                     # every candidate lands far outside: logits 0, uniform
    u = confidence.depth_match_stats(f0, f1, h, w, away, cand, peak_radius=0)
    d = cand.numel()
    assert bool((u.in_view == 0).all()) and bool((u.best == 0).all())
    assert torch.equal(u.max_prob, torch.full_like(u.max_prob, 1.0 / d)) and (u.entropy - math.log(d)).abs().max().item() < 1e-14
    with pytest.raises(ValueError):
        confidence.depth_match_stats(f0, f1, h, w, cam[:1], cand)
    with pytest.raises(ValueError):
        confidence.depth_match_stats(f0, f1, h, w, cam, cand, peak_radius=-1)


def test_abi_argument_checks_without_a_gpu():
    lib = _abi.load()
    p = 0x1000                                   # never dereferenced: every call below fails its argument checks first

    def call(f0=p, f1=p, cam=p, cand=p, out=p, stats=p, index=p, batch=2, h=6, w=8, c=128, d=16, argmax=0, radius=1):
        return lib.um_depth_corr_softmax_stats(f0, f1, cam, cand, out, stats, index, batch, h, w, c, d, argmax, radius, None)

    def message():
        return lib.um_last_error_string().decode()

    for null in ('f0', 'f1', 'cam', 'cand', 'out'):
        assert call(**{null: None}) < 0 and 'null pointer' in message(), null
    assert call(c=96) < 0 and 'channels=96' in message()
    assert call(d=0) < 0 and 'num_candidates=0' in message()
    assert call(d=129) < 0 and 'num_candidates=129' in message()
    assert call(radius=-1) < 0 and 'peak_radius=-1' in message()
    assert call(batch=0) < 0 and call(h=0) < 0


# ------------------------------------------------------------------ the model with the oracle backend
def _model(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    return model, dict(fk)


def _frames(count, h, w, seed):
    x = synth_frames(count, h, w, seed=seed) / 255.
    return ((x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).contiguous()


def _host_stats_of_taps(taps, intrinsics, pose, kw, bidir, scale, peak_radius):
    tok0, tok1 = (taps[n].flatten(2).transpose(1, 2).contiguous() for n in ('f0_s0', 'f1_s0'))
    h, w = taps['f0_s0'].shape[-2:]
    k = intrinsics.clone()
    k[:, :2] = k[:, :2] / scale
    if bidir:
        tok0, tok1 = torch.cat([tok0, tok1], 0), torch.cat([tok1, tok0], 0)
        k, pose = k.repeat(2, 1, 1), torch.cat([pose, torch.inverse(pose)], 0)
    cand = torch.linspace(kw.get('min_depth', 1. / 0.5), kw.get('max_depth', 1. / 10), kw.get('num_depth_candidates', 64)).float()
    return confidence.depth_match_stats_host(tok0, tok1, h, w, _cam(k, pose).float(), cand, peak_radius), h, w


@pytest.mark.parametrize('bidir', [False, True])
def test_forward_with_depth_confidence_on_the_host(bidir):
    model, kw = _model('gmdepth_s1')
    x = _frames(3, 64, 96, 2110)
    img0, img1 = x[:2], x[1:]
    k, rel = synth_camera(2, 64, 96)
    kw = dict(kw, intrinsics=k, pose=rel, pred_bidir_depth=bidir)
    plain = model(img0, img1, **kw)
    model.debug_taps = taps = {}
    out = model.forward_with_depth_confidence(img0, img1, peak_radius=2, **kw)
    model.debug_taps = None
    assert set(out) == set(plain) | {'depth_confidence'}
    assert all(torch.equal(a, b) for a, b in zip(out['flow_preds'], plain['flow_preds']))
    conf = out['depth_confidence']
    want, h, w = _host_stats_of_taps(taps, k, rel, kw, bidir, 8, 2)
    assert set(conf) == {'max_prob', 'entropy', 'variance', 'peak_mass', 'best', 'in_view', 'scale', 'num_candidates'}
    assert conf['scale'] == 8 and conf['num_candidates'] == 64 and (h, w) == (8, 12)
    for key in FLOATS + ('best', 'in_view'):
        assert tuple(conf[key].shape) == (4 if bidir else 2, h, w), key
        assert conf[key].dtype == (torch.float32 if key in FLOATS else torch.int32), key
        assert torch.equal(conf[key], getattr(want, key)), key
    assert 'depth_confidence' not in model(img0, img1, **kw)              # forward itself is untouched
    with pytest.raises(ValueError, match='peak_radius'):
        model.forward_with_depth_confidence(img0, img1, peak_radius=-1, **kw)


def test_forward_with_depth_confidence_is_for_depth_only():
    model, kw = _model('gmflow_s1')
    frames = synth_frames(2, 64, 96, seed=2111)
    with pytest.raises(ValueError, match="task='depth'"):
        model.forward_with_depth_confidence(frames[:1], frames[1:], **kw)
    model, kw = _model('gmdepth_s1')
    with pytest.raises(NotImplementedError, match='plane sweep.*forward_with_depth_confidence'):
        model.forward_with_confidence(frames[:1], frames[1:], intrinsics=torch.eye(3)[None], pose=torch.eye(4)[None], **kw)


def test_forward_sequence_returns_the_depth_confidence_of_its_own_forward():
    """Chunks of two pairs with a carry give what the pairwise ``forward_with_depth_confidence`` gives, in the forward direction, and
    the depths are those of the plain sequence call bit for bit."""
    model, kw = _model('gmdepth_s1')
    kw.pop('task')
    x = _frames(4, 64, 96, 2112)
    k, rel = synth_camera(1, 64, 96)
    step = torch.linalg.inv(rel[0].double())
    poses = [torch.eye(4, dtype=torch.float64)]
    for _ in range(3):
        poses.append(poses[-1] @ step)
    poses = torch.stack(poses, 0).float()
    pair_pose = torch.linalg.inv(poses[1:]) @ poses[:-1]
    want = model.forward_with_depth_confidence(x[:-1], x[1:], task='depth', intrinsics=k.expand(3, 3, 3), pose=pair_pose,
                                               pred_bidir_depth=True, peak_radius=1, **kw)['depth_confidence']
    args = dict(task='depth', intrinsics=k, poses=poses, pairs_per_launch=2, pred_bidir_depth=True, **kw)
    plain = model.forward_sequence(x, **args)
    out = model.forward_sequence(x, return_confidence=True, peak_radius=1, **args)
    assert 'depth_confidence' not in plain and set(out) == set(plain) | {'depth_confidence'}
    assert torch.equal(out['depth'], plain['depth']) and torch.equal(out['depth_bwd'], plain['depth_bwd'])
    conf = out['depth_confidence']
    assert set(conf) == set(want) and conf['scale'] == 8 and conf['num_candidates'] == 64
    # the sequence encodes 3 + 1 frames, the pairwise call 2 x 3: CPU convolutions re-associate with the batch size (a few fp32 ulps on
    # the features, tests/test_video_cpu.py::close), so the maps agree to 1e-4 of their range and the arg-max away from near-ties
    for key in FLOATS:
        assert tuple(conf[key].shape) == (3, 8, 12)
        assert (conf[key] - want[key][:3]).abs().max().item() <= 1e-4 * max(1.0, want[key].abs().max().item()), key
    assert conf['best'].dtype == torch.int32 and (conf['best'] == want['best'][:3]).float().mean() >= 0.98
    assert conf['in_view'].dtype == torch.int32 and (conf['in_view'] == want['in_view'][:3]).float().mean() >= 0.98
    with pytest.raises(ValueError, match='peak_radius'):
        model.forward_sequence(x, return_confidence=True, peak_radius=-2, **args)


# ------------------------------------------------------------------ the fused point cloud
def test_fuse_depth_sequence_filters_on_confidence():
    t, h, w = 3, 12, 16
    g = torch.Generator().manual_seed(5)
    depths = 2.0 + 0.2 * torch.rand(t, h, w, generator=g)
    k = torch.tensor([[[14.0, 0, 7.5], [0, 14.0, 5.5], [0, 0, 1]]])
    poses = torch.eye(4).repeat(t, 1, 1)
    poses[:, 0, 3] = torch.arange(t) * 0.01
    colors = (torch.rand(t, h, w, 3, generator=g) * 255).to(torch.uint8)
    args = dict(px_thr=50.0, rel_thr=1.0)                                  # loose: the consistency check keeps nearly everything
    base = geometry.fuse_depth_sequence(depths, k, poses, colors, **args)
    conf = torch.full((t, h, w), 0.9)
    same = geometry.fuse_depth_sequence(depths, k, poses, colors, confidence=conf, **args)                 # min_confidence = 0
    for key in ('keep', 'xyz', 'rgb'):
        assert torch.equal(base[key], same[key]), key
    conf[1, 3:7, 4:10] = 0.2                                               # a planted low-confidence rectangle in frame 1
    out = geometry.fuse_depth_sequence(depths, k, poses, colors, confidence=conf, min_confidence=0.5, **args)
    want = base['keep'].clone()
    want[1, 3:7, 4:10] = 0
    assert base['keep'][1, 3:7, 4:10].sum() > 0 and torch.equal(out['keep'], want)
    assert out['xyz'].shape[0] == int(want.sum().item()) == base['xyz'].shape[0] - int(base['keep'][1, 3:7, 4:10].sum().item())
    with pytest.raises(ValueError, match='confidence'):
        geometry.fuse_depth_sequence(depths, k, poses, colors, confidence=conf[:, :4], **args)


def test_confidence_to_image_size_upsamples_and_restores():
    from unimatch_amd.prepost import InferenceGeometry
    m = torch.arange(6, dtype=torch.float32).view(1, 2, 3) / 6
    up = confidence.confidence_to_image_size(m, 8)
    assert tuple(up.shape) == (1, 16, 24) and torch.equal(up[0, ::8, ::8], m[0]) and torch.equal(up[0, :8, :8], torch.full((8, 8), 0.0))
    geom = InferenceGeometry.resized((12, 20), (16, 24))
    back = confidence.confidence_to_image_size(m, 8, geom)
    assert tuple(back.shape) == (1, 12, 20) and back.min() >= 0 and back.max() <= m.max()       # resized, values not rescaled


# ------------------------------------------------------------------ the scene driver
@pytest.mark.parametrize('step', [None, 2])
def test_run_depth_writes_confidence_and_filters_the_cloud(tmp_path, monkeypatch, step):
    """``--save-confidence`` / ``--min-confidence`` through the pairwise path (``step=None``) and the ``--pairs-per-launch`` path: one
    ``<stem>_conf.png`` per depth map at the frames' size, the plain outputs unchanged, and the fused cloud filtered on ``peak_mass`` at
    image size with the given threshold."""
    pil = pytest.importorskip('PIL.Image')
    from unimatch_amd import depth
    from unimatch_amd.prepost import InferenceGeometry
    from tests.test_depth_sequence_cpu import write_scene
    h, w = 24, 40
    names = [f'{i:04d}.png' for i in (0, 20, 40)]
    images = write_scene(tmp_path / 'scene', names, h, w)
    model, kw = _model('gmdepth_s1')
    common = dict(padding_factor=16, min_depth=0.5, max_depth=10., num_depth_candidates=16, device='cpu', pairs_per_launch=step)
    seen = {}
    fuse = geometry.fuse_depth_sequence

    def recording(*a, **k):
        seen.update(k)
        return fuse(*a, **k)

    monkeypatch.setattr(geometry, 'fuse_depth_sequence', recording)
    assert depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'plain'), kw, save_ply=str(tmp_path / 'plain.ply'), **common) == 2
    assert 'confidence' not in seen and not os.path.exists(tmp_path / 'plain' / '0000_conf.png')
    assert depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'conf'), kw, save_ply=str(tmp_path / 'conf.ply'), save_confidence=True,
                           min_confidence=0.4, peak_radius=2, **common) == 2
    assert sorted(os.listdir(tmp_path / 'conf')) == ['0000.png', '0000_conf.png', '0020.png', '0020_conf.png']
    for stem in ('0000', '0020'):
        assert np.array(pil.open(tmp_path / 'conf' / f'{stem}_conf.png')).shape == (h, w, 3)
        assert np.array_equal(np.array(pil.open(tmp_path / 'conf' / f'{stem}.png')), np.array(pil.open(tmp_path / 'plain' / f'{stem}.png')))
    assert seen['min_confidence'] == 0.4 and tuple(seen['confidence'].shape) == (2, h, w)
    assert 0 <= seen['confidence'].min() and seen['confidence'].max() <= 1 + 1e-6
    # frame 0's map is the pairwise method's peak_mass at radius 2, brought to the frame's size
    imgs, poses, k = depth.read_scene(str(tmp_path / 'scene'))
    geom = InferenceGeometry.resized((h, w), (32, 48))
    a = geom.prepare(torch.from_numpy(np.stack(images, 0)), normalize=True)[0]
    pose = torch.from_numpy(depth.relative_pose(poses[0], poses[1]))[None]
    out = model.forward_with_depth_confidence(a[:1], a[1:2], peak_radius=2, intrinsics=torch.from_numpy(k)[None], pose=pose,
                                              **dict(kw, min_depth=1 / 10., max_depth=1 / 0.5, num_depth_candidates=16))
    conf = out['depth_confidence']
    want = confidence.confidence_to_image_size(conf['peak_mass'], conf['scale'], geom)[0]
    assert (seen['confidence'][0] - want).abs().max().item() <= (0 if step is None else 1e-4)
    if step is None:
        max_prob = torch.cat([conf['max_prob'], model.forward_with_depth_confidence(
            a[1:2], a[2:3], peak_radius=2, intrinsics=torch.from_numpy(k)[None],
            pose=torch.from_numpy(depth.relative_pose(poses[1], poses[2]))[None],
            **dict(kw, min_depth=1 / 10., max_depth=1 / 0.5, num_depth_candidates=16))['depth_confidence']['max_prob']], 0)
    else:                                                                  # the sequence call the driver makes, repeated
        seq = model.forward_sequence(a, intrinsics=torch.from_numpy(k)[None], poses=torch.from_numpy(poses), pairs_per_launch=step,
                                     return_confidence=True, peak_radius=2,
                                     **dict(kw, min_depth=1 / 10., max_depth=1 / 0.5, num_depth_candidates=16))
        max_prob = seq['depth_confidence']['max_prob']
    rgb = confidence.confidence_to_image(max_prob, (h, w)).numpy()
    for j, stem in enumerate(('0000', '0020')):
        assert np.array_equal(np.array(pil.open(tmp_path / 'conf' / f'{stem}_conf.png')), rgb[j]), stem
    with pytest.raises(ValueError, match='save_ply'):
        depth.run_depth(model, str(tmp_path / 'scene'), str(tmp_path / 'x'), kw, min_confidence=0.5, **common)
