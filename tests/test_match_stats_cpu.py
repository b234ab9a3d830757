"""CPU tests of the matching confidence (``unimatch_amd.confidence``): the host restatement against the ``prob`` the reference returns
(tests/golden/match_stats.npz), the exact single-key row, the mutual check on a hand-built permutation, the C ABI's argument checks
without a GPU, and ``UniMatch.forward_with_confidence`` with the CPU oracle injected as hot-path backend."""
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, confidence
from unimatch_amd.synth import CONFIGS, synth_frames, synth_state_dict
from tests.oracle_ops import OracleOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'match_stats.npz')
RTOL, ATOL = 1.3e-6, 1e-5                       # torch.testing.assert_close's float32 defaults
FIELDS = ('max_prob', 'entropy', 'variance', 'mean')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _tokens(m):
    """``[B, C, h, w]`` -> token-major ``[B, h*w, C]`` float32."""
    t = torch.from_numpy(np.asarray(m, dtype=np.float32))
    return t.flatten(2).transpose(1, 2).contiguous()


@pytest.mark.parametrize('case', ['flow', 'flow_bidir', 'stereo'])
def test_host_matches_the_reference_prob(golden, case):
    """``global_match_stats_host`` (float32, on the golden features) against the statistics taken directly from the reference's stored
    float32 ``prob``.  Tolerance per statistic: the larger of assert_close's float32 defaults and 4 x the distance between taking
    those statistics from the stored ``prob`` in float32 and in float64 -- the rounding noise of the derivation itself.  Measured
    noise (max abs, printed below): 0 for max_prob, 1.7e-7 .. 3.9e-7 for the entropy, 8.7e-7 .. 1.4e-6 for the mean and 1.5e-6 ..
    2.0e-6 for the variance; 4 x the largest is 8.1e-6, so the float32 defaults are the binding term everywhere."""
    stereo = case == 'stereo'
    key = 'stereo' if stereo else 'flow'
    f0, f1 = _tokens(golden[f'{key}_f0']), _tokens(golden[f'{key}_f1'])
    h, w = golden[f'{key}_f0'].shape[-2:]
    prob = torch.from_numpy(golden['stereo_prob' if stereo else 'flow_prob_bidir'])
    if case == 'flow':                           # without pred_bidir_flow the reference returns the first half, bit for bit (the generator asserts it)
        prob = prob[:2]
    got = confidence.global_match_stats_host(f0, f1, h, w, bidir=(case == 'flow_bidir'), stereo=stereo)
    ref32 = confidence.stats_from_prob_host(prob, h, w, stereo)
    ref64 = confidence.stats_from_prob_host(prob.double(), h, w, stereo)
    assert got.max_prob.dtype == torch.float32 and got.best.dtype == torch.int32
    assert tuple(got.max_prob.shape) == (prob.shape[0], h, w) and tuple(got.mean.shape) == (prob.shape[0], 1 if stereo else 2, h, w)
    for name in FIELDS:
        g, r32, r64 = getattr(got, name), getattr(ref32, name), getattr(ref64, name)
        noise = (r32.double() - r64).abs().max().item()
        err = (g.double() - r64).abs()
        allowed = torch.clamp(ATOL + RTOL * r64.abs(), min=4 * noise)
        print(f'{case} {name}: derivation noise {noise:.3e}, host error {err.max().item():.3e}')
        assert bool((err <= allowed).all()), (case, name, err.max().item(), noise)
    assert torch.equal(got.best, ref64.best)
    if case == 'flow_bidir':                                               # the second half is the swapped direction
        swapped = confidence.global_match_stats_host(f1, f0, h, w)
        assert torch.equal(got.max_prob[2:], swapped.max_prob) and torch.equal(got.best[2:], swapped.best)
    # the fixture spans flat and peaked rows
    assert ref64.max_prob.min() < 0.2 and ref64.max_prob.max() > 0.9


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_stereo_first_column_is_exactly_certain(golden, dtype):
    f0, f1 = _tokens(golden['stereo_f0']).to(dtype), _tokens(golden['stereo_f1']).to(dtype)
    h, w = golden['stereo_f0'].shape[-2:]
    s = confidence.global_match_stats(f0, f1, h, w, stereo=True)           # host tensors: the host path
    assert bool((s.max_prob[..., 0] == 1).all()) and bool((s.entropy[..., 0] == 0).all()) and bool((s.variance[..., 0] == 0).all())
    assert bool((s.best[..., 0] == 0).all()) and bool((s.mean[..., 0] == 0).all())
    assert bool((s.best <= torch.arange(w)).all())                         # a key never lies right of its query
    assert bool((s.entropy >= 0).all()) and bool((s.variance >= 0).all())


def test_mean_is_the_flow_and_minus_the_disparity(golden):
    """``mean`` restates what the matching entry points return: the reference's own expectation of ``prob``."""
    f0, f1 = _tokens(golden['flow_f0']).double(), _tokens(golden['flow_f1']).double()
    h, w = golden['flow_f0'].shape[-2:]
    prob = torch.from_numpy(golden['flow_prob_bidir'][:2]).double()
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    grid = torch.stack([gx.flatten(), gy.flatten()], -1)
    flow = (prob @ grid - grid).transpose(1, 2).reshape(2, 2, h, w)
    torch.testing.assert_close(confidence.global_match_stats_host(f0, f1, h, w).mean, flow, rtol=0, atol=1e-5)


def test_mutual_matches_on_a_permutation():
    h, w = 3, 4
    l = h * w
    fwd = torch.tensor([1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10], dtype=torch.int32)          # pairwise swaps
    bwd = fwd.clone()                                                                       # its own inverse: all mutual
    bwd[1] = 1            # key 1 prefers itself: query 0 (-> 1 -> 1) misses by one column
    bwd[7] = 0            # key 7 prefers 0: query 6 (-> 7 -> 0) misses by one row and two columns
    bwd[9] = -1           # an invalid index is no match
    m0 = confidence.mutual_matches(fwd.view(1, h, w), bwd.view(1, h, w), h, w, radius=0)
    m1 = confidence.mutual_matches(fwd.view(1, h, w), bwd.view(1, h, w), h, w, radius=1)
    assert m0.dtype == torch.bool and tuple(m0.shape) == (1, h, w)
    expect0 = torch.ones(l, dtype=torch.bool)
    expect0[[0, 6, 8]] = False
    expect1 = expect0.clone()
    expect1[0] = True
    assert torch.equal(m0.flatten(), expect0) and torch.equal(m1.flatten(), expect1)
    with pytest.raises(ValueError):
        confidence.mutual_matches(fwd.view(1, h, w), bwd.view(1, h, w), h, w, radius=-1)
    with pytest.raises(ValueError):
        confidence.mutual_matches(fwd.view(1, h, w), bwd.view(1, w, h), h, w)


def test_abi_argument_checks_without_a_gpu():
    lib = _abi.load()
    assert lib.um_version() == 220
    size = lib.um_global_match_stats_workspace_bytes
    need = size(2, 60, 128, 0)
    assert need == 2 * 2 * (2 * 60 * 128 * 2) and size(2, 60, 128, 1) == need // 2       # two plane sets; exact mode has hi | lo
    assert size(2, 60, 64, 0) == 0 and size(0, 60, 128, 0) == 0 and size(2, 60, 128, 2) == 0
    p = 0x1000                                   # never dereferenced: every call below fails its argument checks first

    def call(f0=p, f1=p, stats=p, best=p, mean=p, batch=2, h=6, w=10, c=128, bidir=0, stereo=0, mode=0, ws=p, ws_bytes=need):
        return lib.um_global_match_stats(f0, f1, stats, best, mean, batch, h, w, c, bidir, stereo, mode, ws, ws_bytes, None)

    def message():
        return lib.um_last_error_string().decode()

    for null in ('f0', 'f1', 'stats', 'best'):
        assert call(**{null: None}) == -1 and 'null pointer' in message()
    assert call(batch=0) == -1 and call(h=0) == -1
    assert call(c=64) == -1 and 'channels=64' in message()
    assert call(mode=2) == -1 and 'mode=2' in message()
    assert call(bidir=1, stereo=1) == -1 and 'bidir' in message() and 'stereo' in message()
    assert call(ws=None) == -3 and call(ws_bytes=need - 1) == -3 and 'workspace too small' in message()
    assert lib.um_match_mutual(None, p, p, 1, 3, 4, 0, None) == -1 and lib.um_match_mutual(p, p, p, 1, 3, 4, -1, None) == -1
    assert 'um_match_mutual' in message()


def test_public_function_rejects_bad_arguments(golden):
    f0, f1 = _tokens(golden['flow_f0']), _tokens(golden['flow_f1'])
    with pytest.raises(ValueError):
        confidence.global_match_stats(f0, f1, 6, 10, bidir=True, stereo=True)
    with pytest.raises(ValueError):
        confidence.global_match_stats(f0, f1, 6, 11)
    with pytest.raises(ValueError):
        confidence.global_match_stats(f0, f1, 6, 10, precision='half')


# ------------------------------------------------------------------ forward_with_confidence with the oracle backend
def _model(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    return model, dict(fk)


@pytest.mark.parametrize('name,bidir', [('gmflow_s1', True), ('gmflow_s1', False), ('gmstereo_s1', False)])
def test_forward_with_confidence_on_the_host(name, bidir):
    model, kw = _model(name)
    if bidir:
        kw['pred_bidir_flow'] = True
    frames = synth_frames(3, 64, 96, seed=2100)
    img0, img1 = frames[:2], frames[1:]
    plain = model(img0, img1, **kw)
    model.debug_taps = taps = {}
    out = model.forward_with_confidence(img0, img1, **kw)
    model.debug_taps = None
    assert set(out) == set(plain) | {'match_confidence'}
    assert all(torch.equal(a, b) for a, b in zip(out['flow_preds'], plain['flow_preds']))
    conf = out['match_confidence']
    h, w = taps['f0_s0'].shape[-2:]
    stereo = kw['task'] == 'stereo'
    want = confidence.global_match_stats_host(taps['f0_s0'].flatten(2).transpose(1, 2), taps['f1_s0'].flatten(2).transpose(1, 2), h, w,
                                              bidir=bidir, stereo=stereo)
    assert conf['scale'] == 8 and (h, w) == (8, 12)
    assert set(conf) == {'max_prob', 'entropy', 'variance', 'best', 'scale'} | ({'mutual'} if bidir else set())
    for key in ('max_prob', 'entropy', 'variance', 'best'):
        assert torch.equal(conf[key], getattr(want, key)), key
    assert tuple(conf['max_prob'].shape) == (4 if bidir else 2, h, w)
    if bidir:
        assert torch.equal(conf['mutual'], confidence.mutual_matches_host(want.best[:2], want.best[2:], h, w, 0))
        assert conf['mutual'].dtype == torch.bool and tuple(conf['mutual'].shape) == (2, h, w)
    # forward itself is untouched: no key appears in its output afterwards
    assert 'match_confidence' not in model(img0, img1, **kw)


def test_forward_with_confidence_refuses_depth_and_local_matching():
    model, kw = _model('gmdepth_s1')
    frames = synth_frames(2, 64, 96, seed=2101)
    with pytest.raises(NotImplementedError, match='plane sweep'):
        model.forward_with_confidence(frames[:1], frames[1:], intrinsics=torch.eye(3)[None], pose=torch.eye(4)[None], **kw)
    model, kw = _model('gmflow_s1')
    with pytest.raises(ValueError, match='global matching'):
        model.forward_with_confidence(frames[:1], frames[1:], **dict(kw, corr_radius_list=[4]))


def test_forward_with_confidence_rejects_bidir_stereo_up_front():
    model, kw = _model('gmstereo_s1')
    frames = synth_frames(2, 64, 96, seed=2101)
    with pytest.raises(ValueError, match='pred_bidir_flow is a flow option'):
        model.forward_with_confidence(frames[:1], frames[1:], pred_bidir_flow=True, **kw)


def test_forward_sequence_returns_the_confidence_of_its_own_forward():
    """``return_confidence``: chunks with a carry give what the pairwise ``forward_with_confidence`` gives, in the forward direction,
    and the flows are those of the plain sequence call bit for bit."""
    model, kw = _model('gmflow_s1')
    kw.pop('task')
    frames = synth_frames(4, 64, 96, seed=2103)
    want = model.forward_with_confidence(frames[:-1], frames[1:], pred_bidir_flow=True, **kw)['match_confidence']
    plain = model.forward_sequence(frames, pred_bidir_flow=True, pairs_per_launch=2, **kw)
    out = model.forward_sequence(frames, pred_bidir_flow=True, pairs_per_launch=2, return_confidence=True, **kw)
    assert 'match_confidence' not in plain and torch.equal(out['flow'], plain['flow']) and torch.equal(out['flow_bwd'], plain['flow_bwd'])
    conf = out['match_confidence']
    assert set(conf) == {'max_prob', 'entropy', 'variance', 'best', 'scale', 'mutual'} and conf['scale'] == 8
    # the sequence encodes 3 + 1 frames, the pairwise call 2 x 3: CPU convolutions re-associate with the batch size (a few fp32 ulps on
    # the features, tests/test_video_cpu.py::close), so the maps agree to 1e-4 of their range and the arg-max away from near-ties
    for key in ('max_prob', 'entropy', 'variance'):
        assert tuple(conf[key].shape) == (3, 8, 12)
        assert (conf[key] - want[key][:3]).abs().max().item() <= 1e-4 * max(1.0, want[key].abs().max().item()), key
    assert conf['best'].dtype == torch.int32 and (conf['best'] == want['best'][:3]).float().mean() >= 0.98
    assert conf['mutual'].dtype == torch.bool and (conf['mutual'] == want['mutual']).float().mean() >= 0.98
    with pytest.raises(ValueError, match='global matching'):
        model.forward_sequence(frames, return_confidence=True, **dict(kw, corr_radius_list=[4]))


# ------------------------------------------------------------------ the frame-directory driver with --save-confidence
@pytest.mark.parametrize('mode', ['wide', 'tall', 'tall_device_resize'])
def test_run_directory_writes_confidence_images(tmp_path, mode):
    """``<stem>_conf.png`` for wide frames, for tall ones (the driver transposes them for the model and the map back) and with the
    device-side geometry doing that transpose."""
    pil = pytest.importorskip('PIL.Image')
    from unimatch_amd import io, video
    model, kw = _model('gmflow_s1')
    kw.pop('task')
    tall = mode != 'wide'
    frames = synth_frames(4, 48, 64, seed=2102)
    if tall:
        frames = frames.transpose(-2, -1)
    size = tuple(frames.shape[-2:])
    (tmp_path / 'in').mkdir()
    for i, f in enumerate(frames):
        io.write_png8(str(tmp_path / 'in' / f'{i:02d}.png'), f.permute(1, 2, 0).clamp(0, 255).byte().numpy())
    paths = video.list_frames(str(tmp_path / 'in'))
    extra = dict(pairs_per_launch=2, device='cpu', device_resize=mode == 'tall_device_resize')
    n = video.run_directory(model, paths, str(tmp_path / 'plain'), kw, **extra)
    m = video.run_directory(model, paths, str(tmp_path / 'conf'), kw, save_confidence=True, **extra)
    assert n == m == 3 and not os.path.exists(tmp_path / 'plain' / '0000_conf.png')
    seq = torch.stack([video.read_frame(p) for p in paths], 0)
    if tall:
        seq = seq.transpose(-2, -1)                                        # what the model is given
    want = model.forward_with_confidence(seq[:-1].contiguous(), seq[1:].contiguous(), **kw)['match_confidence']['max_prob']
    assert tuple(want.shape) == (3, 6, 8)
    rgb = confidence.confidence_to_image(want.transpose(-2, -1) if tall else want, size).numpy()
    for j in range(3):                                                     # the second chunk's pair starts at the carried frame
        got = np.array(pil.open(tmp_path / 'conf' / f'{j:04d}_conf.png'))
        assert got.shape == size + (3,) and np.array_equal(got, rgb[j]), j
        assert np.array_equal(got[:8, :8], np.broadcast_to(got[0, 0], (8, 8, 3)))          # nearest: one colour per feature pixel
        flow = np.array(pil.open(tmp_path / 'conf' / f'{j:04d}_flow.png'))
        assert np.array_equal(flow, np.array(pil.open(tmp_path / 'plain' / f'{j:04d}_flow.png')))
