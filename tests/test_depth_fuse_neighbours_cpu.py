"""CPU tests of the fused sequence mode of posed-video depth (``forward_sequence(task='depth', fuse_neighbours=True)``): the C ABI of
``um_depth_corr_softmax_multi_rows`` without a GPU (nothing is launched), the host restatement on operands named by a row table against
the source-major call, and the model on host tensors with the CPU oracle injected as hot-path backend -- against ``forward_multiview``
per frame (the oracle of the feature), against the unfused sequence for a first frame, and fed in pieces with the carry.

The model comparisons use ``floor_close`` of tests/test_video_gpu.py (1e-3 x max(1, |want|max)): the project's gate for "the same
mathematics in another batch composition"."""
import ctypes

import pytest
import torch

from tests import depth_fuse_neighbours_util as fu
from tests import depth_multiview_util as mv
from tests.test_depth_sequence_cpu import H, NAMES, T, W, _model, host_relative, scene
from tests.test_video_gpu import floor_close
from unimatch_amd import _abi, confidence

CASES = ['A', 'B', 'C', 'D', 'one1']


# ------------------------------------------------------------------ the C ABI
def test_the_library_exports_the_entry_point_and_keeps_its_version():
    lib = _abi.load()
    assert hasattr(lib, 'um_depth_corr_softmax_multi_rows')
    assert 'um_depth_corr_softmax_multi_rows' in _abi.SIGNATURES
    assert lib.um_version() == 220


def test_abi_argument_checks_without_a_gpu():
    lib = _abi.load()
    p = 0x1000                                   # never dereferenced: every call below fails its argument checks first

    def call(segments=(p, p, p), segment_rows=(4, 4, 2), num_segments=None, cam=p, cam_rows=6, rows=p, cand=p, out=p, stats=p, index=p,
             sources=2, batch=2, h=6, w=8, c=128, d=16, argmax=0, radius=1):
        seg = None if segments is None else (ctypes.c_void_p * 4)(*(list(segments) + [None] * (4 - len(segments))))
        cnt = None if segment_rows is None else (ctypes.c_int * 4)(*(list(segment_rows) + [0] * (4 - len(segment_rows))))
        n = len(segments) if num_segments is None else num_segments
        return lib.um_depth_corr_softmax_multi_rows(seg, cnt, n, cam, cam_rows, rows, cand, out, stats, index, sources, batch, h, w, c, d,
                                                    argmax, radius, None)

    def message():
        return lib.um_last_error_string().decode()

    for null in ('segments', 'segment_rows', 'cam', 'rows', 'cand', 'out'):
        kw = {null: None}
        if null == 'segments':
            kw['num_segments'] = 3
        assert call(**kw) < 0 and 'null pointer' in message(), null
    assert call(segments=(p, None, p)) < 0 and 'segment 1' in message()
    assert call(segment_rows=(4, 4, 0)) < 0 and 'segment 2' in message()
    assert call(segment_rows=(4, -1, 2)) < 0 and 'segment 1' in message()
    assert call(num_segments=0) < 0 and 'num_segments=0' in message()
    assert call(segments=(p, p, p, p), segment_rows=(1, 1, 1, 1), num_segments=5) < 0 and 'num_segments=5' in message()
    assert call(cam_rows=0) < 0 and 'cam_rows=0' in message()
    assert call(cam_rows=-3) < 0 and 'cam_rows=-3' in message()
    assert call(c=96) < 0 and 'channels=96' in message()
    assert call(d=0) < 0 and 'num_candidates=0' in message()
    assert call(d=129) < 0 and 'num_candidates=129' in message()
    assert call(sources=0) < 0 and 'sources=0' in message()
    assert call(sources=9) < 0 and 'sources=9' in message()
    assert call(radius=-1) < 0 and 'peak_radius=-1' in message()
    assert call(batch=0) < 0 and call(h=0) < 0 and call(w=0) < 0


# ------------------------------------------------------------------ the host restatement
def _source_major(case, use=None, peak_radius=2):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    logits = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand, use)
    return logits, confidence.depth_match_multi(f0, f1, h, w, cam, cand, use, peak_radius=peak_radius)


@pytest.mark.parametrize('segments', [1, 2, 3, 4])
@pytest.mark.parametrize('case', CASES)
def test_rows_equal_the_source_major_call(case, segments):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, segments, seed=len(case))
    assert len(segs) == segments and all(t.shape[0] >= 1 for t in segs) and bool(torch.isnan(torch.cat(segs, 0)).any())
    want_logits, (want_out, want_stats) = _source_major(case)
    got_logits = confidence.depth_match_logits_multi_host(segs, None, h, w, table, cand, rows=rows)
    assert all(torch.equal(a, e) for a, e in zip(got_logits, want_logits))
    out, stats = confidence.depth_match_multi(segs, None, h, w, table, cand, peak_radius=2, rows=rows)
    assert torch.equal(out, want_out) and all(torch.equal(a, e) for a, e in zip(stats, want_stats))
    st = confidence.depth_match_stats_multi_host(segs, None, h, w, table, cand, peak_radius=2, rows=rows)
    assert all(torch.equal(a, e) for a, e in zip(st, want_stats))
    hard, _ = confidence.depth_match_multi(segs, None, h, w, table, cand, from_argmax=True, rows=rows)
    assert torch.equal(hard, confidence.depth_match_multi(f0, f1, h, w, cam, cand, from_argmax=True)[0])
    conf_out, conf = confidence.depth_match_multi_confidence(None, segs, None, h, w, table, cand, None, False, 8, 2, rows=rows)
    assert torch.equal(conf_out, want_out) and torch.equal(conf['max_prob'], want_stats.max_prob) and conf['scale'] == 8


@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_bad_indices_are_the_use_mask(case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, 3, seed=7)
    total = sum(t.shape[0] for t in segs)
    use = torch.ones(len(moves), b, dtype=torch.bool)
    use[1, 0] = use[0, 1] = False
    if len(moves) > 2:
        use[2, 1] = False                                                # sample 1: source 1 alone is left
    want_logits, (want_out, want_stats) = _source_major(case, use)
    bad = fu.switch_off(rows, use, total, table.shape[0])
    assert int((bad != rows).any(-1).sum()) == int((~use).sum())
    out, stats = confidence.depth_match_multi(segs, None, h, w, table, cand, peak_radius=2, rows=bad)
    assert torch.equal(out, want_out) and all(torch.equal(a, e) for a, e in zip(stats, want_stats))
    # every source of sample 0 off: the uniform distribution, nothing in view
    none = rows.clone()
    none[:, 0, 1] = torch.tensor([-1, total, fu.BIG][:len(moves)], dtype=torch.int32)
    logits, in_view, views = confidence.depth_match_logits_multi_host(segs, None, h, w, table, cand, rows=none)
    assert bool((logits[0] == 0).all()) and bool((in_view[0] == 0).all()) and bool((views[0] == 0).all())
    assert torch.equal(logits[1], _source_major(case)[0][0][1])


def test_rows_refuse_mixed_operands():
    (b, h, w), d, moves = mv.CASES['A']
    f0, f1, cam, cand = mv.inputs('A')
    segs, table, rows = fu.scatter(f0, f1, cam, 2)
    with pytest.raises(ValueError, match='f1 must be None'):
        confidence.depth_match_multi(segs, f1, h, w, table, cand, rows=rows)
    with pytest.raises(ValueError, match='use must be None'):
        confidence.depth_match_multi(segs, None, h, w, table, cand, torch.ones(2, b, dtype=torch.uint8), rows=rows)
    with pytest.raises(ValueError, match='segments'):
        confidence.depth_match_multi(segs[0], None, h, w, table, cand, rows=rows)
    with pytest.raises(ValueError, match='segments'):
        confidence.depth_match_multi(segs * 3, None, h, w, table, cand, rows=rows)
    with pytest.raises(ValueError, match='rows'):
        confidence.depth_match_multi(segs, None, h, w, table, cand, rows=rows[..., :2])
    with pytest.raises(ValueError, match='cam'):
        confidence.depth_match_multi(segs, None, h, w, cam, cand, rows=rows)         # the source-major cam [S, B, 30]


# ------------------------------------------------------------------ the model with the oracle backend
@pytest.fixture(scope='module', params=NAMES)
def seq(request):
    model, kw = _model(request.param)
    x, k, poses = scene()
    args = dict(task='depth', intrinsics=k, **kw)
    plain = model.forward_sequence(x, poses=poses, pairs_per_launch=2, **args)
    fused = model.forward_sequence(x, poses=poses, pairs_per_launch=2, fuse_neighbours=True, **args)
    return model, kw, x, k, poses, args, plain, fused


def test_keys_shapes_and_the_default(seq):
    model, kw, x, k, poses, args, plain, fused = seq
    assert set(fused) == {'depth', 'carry'} and tuple(fused['depth'].shape) == (T - 1, H, W) and bool(torch.isfinite(fused['depth']).all())
    assert set(fused['carry']) == {'features', 'frame', 'state', 'pose', 'intrinsics', 'neighbour'}
    nbr = fused['carry']['neighbour']
    assert set(nbr) == {'tokens', 'pose', 'intrinsics'} and tuple(nbr['tokens'].shape) == (2, (H // 8) * (W // 8), 128)
    assert torch.equal(nbr['pose'], host_relative(poses)[-1:]) and torch.equal(nbr['intrinsics'], k)
    off = model.forward_sequence(x, poses=poses, pairs_per_launch=2, fuse_neighbours=False, **args)
    assert set(off) == set(plain) == {'depth', 'carry'} and torch.equal(off['depth'], plain['depth'])
    assert set(off['carry']) == set(plain['carry']) == {'features', 'frame', 'state', 'pose', 'intrinsics'}
    more = model.forward_sequence(x, poses=poses, pairs_per_launch=2, fuse_neighbours=True, colorize=True, return_confidence=True,
                                  peak_radius=2, **args)
    assert set(more) == {'depth', 'depth_rgb', 'depth_confidence', 'carry'} and torch.equal(more['depth'], fused['depth'])
    assert tuple(more['depth_rgb'].shape) == (T - 1, H, W, 3) and more['depth_rgb'].dtype == torch.uint8
    conf = more['depth_confidence']
    assert set(conf) == {'max_prob', 'entropy', 'variance', 'peak_mass', 'best', 'in_view', 'scale', 'num_candidates'}
    for key in ('max_prob', 'entropy', 'variance', 'peak_mass', 'best', 'in_view'):
        assert tuple(conf[key].shape) == (T - 1, H // 8, W // 8), key
    # the union of two views sees at least what one sees; source 0's coordinates are computed identically
    one = model.forward_sequence(x, poses=poses, pairs_per_launch=2, return_confidence=True, peak_radius=2, **args)['depth_confidence']
    assert bool((conf['in_view'] >= one['in_view']).all()) and torch.equal(conf['in_view'][0], one['in_view'][0])


def test_interior_frames_match_forward_multiview_and_frame_zero_the_unfused_sequence(seq):
    model, kw, x, k, poses, args, plain, fused = seq
    rel = host_relative(poses)
    for step in (2, 8, 1):
        got = fused['depth'] if step == 2 else model.forward_sequence(x, poses=poses, pairs_per_launch=step, fuse_neighbours=True,
                                                                      **args)['depth']
        for t in range(1, T - 1):
            srcs = torch.stack([x[t + 1], x[t - 1]], 0)[None]
            pose = torch.stack([rel[t], torch.linalg.inv(rel[t - 1])], 0)[None]
            want = model.forward_multiview(x[t:t + 1], srcs, intrinsics=k, poses=pose, **kw)['flow_preds'][0][0]
            floor = 1e-3 * max(1.0, want.abs().max().item())
            print(f'pairs_per_launch={step} frame {t}: |fused - multiview| {(got[t] - want).abs().max().item():.3e}, '
                  f'|unfused - multiview| {(plain["depth"][t] - want).abs().max().item():.3e}, floor {floor:.3e}')
            assert floor_close(got[t], want), (step, t)
        print(f'pairs_per_launch={step} frame 0: |fused - unfused| {(got[0] - plain["depth"][0]).abs().max().item():.3e}')
        assert floor_close(got[0], plain['depth'][0]), step


def test_pieces_joined_by_the_carry_equal_one_call(seq):
    model, kw, x, k, poses, args, plain, fused = seq
    more = dict(args, pairs_per_launch=2, fuse_neighbours=True, return_confidence=True)
    whole = model.forward_sequence(x, poses=poses, **more)
    a = model.forward_sequence(x[:3], poses=poses[:3], **more)
    b = model.forward_sequence(x[3:], poses=poses[3:], carry=a['carry'], **more)
    assert a['depth'].shape[0] == 2 and b['depth'].shape[0] == 2
    assert torch.equal(torch.cat([a['depth'], b['depth']], 0), whole['depth']) and torch.equal(whole['depth'], fused['depth'])
    for key in ('max_prob', 'in_view', 'best'):
        assert torch.equal(torch.cat([a['depth_confidence'][key], b['depth_confidence'][key]], 0), whole['depth_confidence'][key]), key
    assert all(torch.equal(b['carry']['neighbour'][key], whole['carry']['neighbour'][key]) for key in ('tokens', 'pose', 'intrinsics'))


def test_a_carry_without_the_flag_or_a_stale_one_is_a_first_frame(seq):
    model, kw, x, k, poses, args, plain, fused = seq
    more = dict(args, pairs_per_launch=2)
    first = model.forward_sequence(x[2:], poses=poses[2:], fuse_neighbours=True, **more)['depth']      # frame 2 with source 1 off
    assert floor_close(first[0], plain['depth'][2]) and not floor_close(first[0], fused['depth'][2])
    a = model.forward_sequence(x[:3], poses=poses[:3], **more)
    assert 'neighbour' not in a['carry']
    b = model.forward_sequence(x[3:], poses=poses[3:], carry=a['carry'], fuse_neighbours=True, **more)
    assert floor_close(b['depth'][0], first[0]) and floor_close(b['depth'][1], first[1])
    assert 'neighbour' in b['carry']
    # stale: the carry of a fused call whose model has changed since (a parameter version) -- its frame is encoded again, source 1 off
    a = model.forward_sequence(x[:3], poses=poses[:3], fuse_neighbours=True, **more)
    p = next(model.parameters())
    with torch.no_grad():
        p.add_(0.0)
    assert not model._carry_valid(a['carry'], x[3:])
    b = model.forward_sequence(x[3:], poses=poses[3:], carry=a['carry'], fuse_neighbours=True, **more)
    assert floor_close(b['depth'][0], first[0]) and floor_close(b['depth'][1], first[1])


def test_refusals(seq):
    model, kw, x, k, poses, args, plain, fused = seq
    with pytest.raises(ValueError, match='fuse_neighbours'):
        model.forward_sequence(x, fuse_neighbours=True, attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1])
    with pytest.raises(ValueError, match='pred_bidir_depth'):
        model.forward_sequence(x, poses=poses, fuse_neighbours=True, pred_bidir_depth=True, **args)


# ------------------------------------------------------------------ the runner
def test_the_runner_passes_the_flag_and_refuses_what_the_model_refuses(tmp_path):
    from unimatch_amd import depth

    class StandIn:
        """Records the keywords of every ``forward_sequence`` call; returns constant depths and a carry."""
        def __init__(self):
            self.calls = []

        def forward_sequence(self, frames, carry=None, **kw):
            self.calls.append(dict(kw, carried=carry is not None))
            pairs = frames.shape[0] - (0 if carry is not None else 1)
            return {'depth': torch.full((pairs,) + tuple(frames.shape[2:]), 2.0), 'carry': {'n': len(self.calls)}}

    names = [f'{i:03d}.png' for i in range(4)]
    saved = depth.read_scene, depth.read_frame_u8
    depth.read_scene = lambda scene_dir: (names, torch.eye(4)[None].repeat(4, 1, 1).numpy(), torch.eye(3).numpy())
    depth.read_frame_u8 = lambda path: torch.zeros(32, 48, 3, dtype=torch.uint8)
    try:
        model = StandIn()
        assert depth.run_depth(model, 'scene', str(tmp_path), {}, device='cpu', pairs_per_launch=2, fuse_neighbours=True) == 3
        assert [c['fuse_neighbours'] for c in model.calls] == [True, True] and [c['carried'] for c in model.calls] == [False, True]
        model = StandIn()
        depth.run_depth(model, 'scene', str(tmp_path), {}, device='cpu', pairs_per_launch=2)
        assert all('fuse_neighbours' not in c for c in model.calls)                       # the default launches what it launched before
        with pytest.raises(ValueError, match='pairs_per_launch'):
            depth.run_depth(model, 'scene', str(tmp_path), {}, device='cpu', fuse_neighbours=True)
        with pytest.raises(ValueError, match='pred_bidir_depth'):
            depth.run_depth(model, 'scene', str(tmp_path), {}, device='cpu', pairs_per_launch=2, pred_bidir_depth=True, fuse_neighbours=True)
    finally:
        depth.read_scene, depth.read_frame_u8 = saved
    for argv in (['--scene', 'a', '--out', 'b', '--fuse-neighbours'],
                 ['--scene', 'a', '--out', 'b', '--fuse-neighbours', '--pairs-per-launch', '4', '--pred-bidir-depth']):
        with pytest.raises(SystemExit):
            depth.main(argv)
