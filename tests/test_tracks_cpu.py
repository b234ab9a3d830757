"""CPU tests of the point tracks: the host path of ``video.chain_flows`` against the reference's composition of flows
(tests/golden/tracks.npz) and an fp64 restatement, chunking, the start grid, sparse points, argument errors of the function and of
``um_flow_chain`` (the library loads without a GPU), and the ``track_points`` keyword of ``UniMatch.forward_sequence`` with the CPU
oracle injected as hot-path backend."""
import ctypes
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, video
from unimatch_amd.synth import CONFIGS, synth_frames, synth_state_dict
from tests import tracks_util as tu
from tests.oracle_ops import OracleOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tracks.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_host_chain_matches_reference_composition(golden, tag):
    fwd, comp = torch.from_numpy(golden[f'fwd_{tag}']), torch.from_numpy(golden[f'comp_{tag}'])
    assert all(golden[k].dtype == np.float32 for k in golden.files)
    tracks, visible = video.chain_flows(fwd)
    assert tracks.dtype == torch.float32 and visible.dtype == torch.bool
    tu.check_composition(tracks, visible, comp, *fwd.shape[2:])


def test_generator_and_masks_match_the_minted_inputs(golden):
    """The inputs of the fp64 comparisons are the ones the fixture was minted from, and their masks are the reference's."""
    for tag, (P, h, w, seed) in (('a', (8, 33, 47, 3)), ('b', (6, 64, 97, 4))):
        fwd, occ = tu.inputs(P, h, w, seed)
        assert np.allclose(fwd.numpy(), golden[f'fwd_{tag}'], rtol=0, atol=1e-5)
        assert (occ.numpy() != golden[f'occ_fwd_{tag}']).mean() < 2e-3            # a pixel at the threshold may flip with the warp
    fwd, bwd = torch.from_numpy(golden['fwd_a']), torch.from_numpy(golden['bwd_a'])
    assert np.array_equal(video.forward_backward_consistency_check(fwd, bwd)[0].numpy(), golden['occ_fwd_a'])
    assert (tu.backward_flows(fwd, 3) - bwd).abs().max().item() < 1e-4


@pytest.mark.parametrize('case', tu.CASES, ids=lambda c: 'x'.join(map(str, c[:3])))
def test_host_float32_against_fp64(case):
    P, h, w, seed, mask = case
    fwd, occ = tu.inputs(*case)
    want = tu.chain_fp64(fwd, occ)
    tracks, visible = video.chain_flows(fwd, occ)
    worst = tu.accept(tracks, visible, want)
    end = want[1][-1].float().mean().item()
    print(f'{P}x{h}x{w}: max |d| {worst:.3e} px, occluded {0.0 if occ is None else occ.mean().item():.1%}, alive at the end {end:.1%}')
    if mask:
        assert 0.05 < occ.mean().item() < 0.5 and 0.01 < end < 0.9           # both branches of both tests are exercised


def test_chunks_continue_from_the_last_row():
    fwd, occ = tu.inputs(8, 33, 47, 3)
    tracks, visible = video.chain_flows(fwd, occ)
    t3, v3 = video.chain_flows(fwd[:3], occ[:3])
    t5, v5 = video.chain_flows(fwd[3:], occ[3:], points=t3[-1], alive=v3[-1])
    assert torch.equal(torch.cat([t3, t5], 0), tracks) and torch.equal(torch.cat([v3, v5], 0), visible)
    assert not visible[-1].all() and visible[-1].any()
    # a lost track keeps the position of the step that lost it
    lost = (~visible).float().argmax(0)
    for i in torch.nonzero(~visible[-1]).flatten()[:50].tolist():
        assert torch.equal(tracks[lost[i]:, i], tracks[lost[i], i].expand(tracks.shape[0] - lost[i], 2))


def test_stride_grid_layout():
    fwd, _ = tu.inputs(8, 33, 47, 3)
    zero = torch.zeros_like(fwd[:1])
    tracks, visible = video.chain_flows(zero, stride=3)
    assert tuple(tracks.shape) == (1, 11 * 16, 2) and visible.all()
    grid = tracks[0].view(11, 16, 2)
    assert torch.equal(grid[..., 0], (torch.arange(16.) * 3).expand(11, 16))
    assert torch.equal(grid[..., 1], (torch.arange(11.) * 3)[:, None].expand(11, 16))
    assert torch.equal(tracks[0], video.start_grid(33, 47, 3))
    # the strided tracks are the dense ones at those pixels
    dense, dv = video.chain_flows(fwd)
    some, sv = video.chain_flows(fwd, stride=3)
    pick = (torch.arange(0, 33, 3)[:, None] * 47 + torch.arange(0, 47, 3)).flatten()
    assert torch.equal(some, dense[:, pick]) and torch.equal(sv, dv[:, pick])


def test_sparse_points():
    fwd, occ = tu.inputs(6, 64, 97, 4)
    pts, dead = tu.sparse_points(64, 97)
    assert pts.shape[0] == 257 and torch.isnan(pts).any() and (pts[:, 0] == 96.0).sum() >= 8
    tracks, visible = video.chain_flows(fwd, occ, points=pts)
    assert not visible[:, dead].any()
    frozen = torch.nan_to_num(pts[dead], nan=7.0, posinf=8.0)
    assert all(torch.equal(torch.nan_to_num(row[dead], nan=7.0, posinf=8.0), frozen) for row in tracks)
    assert visible[0, ~dead].float().mean() > 0.5
    tu.accept(tracks, visible, tu.chain_fp64(fwd, occ, points=pts))
    # the alive flags of the caller are honoured
    off = torch.ones(257, dtype=torch.bool)
    off[100:120] = False
    t2, v2 = video.chain_flows(fwd, occ, points=pts, alive=off)
    assert not v2[:, 100:120].any() and torch.equal(t2[-1, 100:120], pts[100:120])
    keep = off & ~dead
    assert torch.equal(t2[:, keep], tracks[:, keep]) and torch.equal(v2[:, keep], visible[:, keep])


def test_chain_flows_argument_errors():
    fwd, occ = tu.inputs(3, 5, 3, 6, False)[0], torch.zeros(3, 5, 3)
    for name, kw in (('flow', dict(flow=fwd[0])), ('flow', dict(flow=fwd[:, :1])), ('flow', dict(flow=fwd.long())),
                     ('flow', dict(flow=fwd[:, :, :1])), ('occ', dict(occ=occ[:2])), ('occ', dict(occ=occ.bool())),
                     ('points', dict(points=torch.zeros(4, 3))), ('points', dict(points=torch.zeros(4, 2, dtype=torch.long))),
                     ('points', dict(points=torch.zeros(0, 2))), ('alive', dict(points=torch.zeros(4, 2), alive=torch.ones(5, dtype=torch.bool))),
                     ('alive', dict(alive=torch.ones(15))), ('stride', dict(stride=0)), ('stride', dict(stride=1.5))):
        args = dict(flow=fwd)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            video.chain_flows(**args)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match='occ'):
            video.chain_flows(fwd.cuda(), occ)


def test_flow_chain_abi_argument_errors_without_gpu():
    lib = _abi.load()
    assert lib.um_version() == 220
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'unimatch_hip.h')).read()
    assert 'um_flow_chain(' in text and 'um_flow_chain' in _abi.SIGNATURES
    p = ctypes.c_void_p(64)
    bad = (
        (None, None, None, None, p, p, 2, 8, 8, 64, 1),            # no flow
        (p, None, None, None, None, p, 2, 8, 8, 64, 1),            # no tracks
        (p, None, None, None, p, None, 2, 8, 8, 64, 1),            # no flags
        (p, None, None, None, p, p, 2, 1, 8, 8, 1),                # h = 1
        (p, None, None, None, p, p, 2, 8, 1, 8, 1),                # w = 1
        (p, None, p, None, p, p, 2, 8, 8, 0, 1),                   # no track
        (p, None, None, None, p, p, 0, 8, 8, 64, 1),               # no pair
        (p, None, None, None, p, p, 2, 8, 8, 63, 1),               # the dense grid has 64 points
        (p, None, None, None, p, p, 2, 8, 8, 64, 3),               # the stride-3 grid has 9
        (p, None, None, None, p, p, 2, 8, 8, 64, 0),               # no stride
        (p, None, None, None, p, p, 2, 1 << 15, 1 << 16, 64, 1),   # h * w beyond 2^30
        (p, None, p, None, p, p, 1 << 20, 8, 8, 1 << 20, 1),       # pairs * n beyond 2^30
    )
    for args in bad:
        assert lib.um_flow_chain(*args, None) == -1, args
        assert b'um_flow_chain' in lib.um_last_error_string()
    assert b'grid' in lib.um_last_error_string() or b'n=' in lib.um_last_error_string()


# ------------------------------------------------------------------ forward_sequence(track_points=...) with the oracle backend
@pytest.fixture(scope='module')
def seq():
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    return model, {k: v for k, v in fk.items() if k != 'task'}, synth_frames(5, 64, 96, seed=2000)


def test_sequence_tracks_equal_chain_of_its_flows(seq):
    model, kw, frames = seq
    plain = model.forward_sequence(frames, pairs_per_launch=3, **kw)
    assert set(plain) == {'flow', 'carry'} and set(plain['carry']) == {'features', 'frame', 'state'}
    out = model.forward_sequence(frames, pairs_per_launch=3, track_points=8, **kw)
    assert set(out) == {'flow', 'tracks', 'tracks_visible', 'carry'} and set(out['carry']) == {'features', 'frame', 'state', 'track'}
    assert torch.equal(out['flow'], plain['flow'])
    assert tuple(out['tracks'].shape) == (4, 8 * 12, 2) and out['tracks_visible'].dtype == torch.bool
    tracks, visible = video.chain_flows(out['flow'], out.get('occ_fwd'), stride=8)
    assert torch.equal(out['tracks'], tracks) and torch.equal(out['tracks_visible'], visible)
    # with both directions the chunk's forward mask ends tracks, and it is the mask consistency_check returns
    both = model.forward_sequence(frames, pairs_per_launch=3, pred_bidir_flow=True, consistency_check=True, track_points='dense', **kw)
    tracks, visible = video.chain_flows(both['flow'], both['occ_fwd'])
    assert torch.equal(both['tracks'], tracks) and torch.equal(both['tracks_visible'], visible)
    quiet = model.forward_sequence(frames, pairs_per_launch=3, pred_bidir_flow=True, track_points='dense', **kw)
    assert 'occ_fwd' not in quiet and torch.equal(quiet['tracks'], tracks) and torch.equal(quiet['tracks_visible'], visible)


def test_sequence_tracks_cross_calls_through_the_carry(seq):
    model, kw, frames = seq
    pts = torch.tensor([[3.0, 4.0], [95.0, 63.0], [40.5, 20.25], [-1.0, 5.0]])
    args = dict(pairs_per_launch=8, pred_bidir_flow=True, **kw)
    whole = model.forward_sequence(frames, track_points=pts, **args)
    assert tuple(whole['tracks'].shape) == (4, 4, 2) and not whole['tracks_visible'][:, 3].any()
    a = model.forward_sequence(frames[:3], track_points=pts, **args)
    b = model.forward_sequence(frames[3:], carry=a['carry'], track_points='dense', **args)      # the value only enables tracking
    flows = torch.cat([a['flow'], b['flow']], 0)
    occ = video.forward_backward_consistency_check(flows, torch.cat([a['flow_bwd'], b['flow_bwd']], 0))[0]
    tracks, visible = video.chain_flows(flows, occ, points=pts)
    assert torch.equal(torch.cat([a['tracks'], b['tracks']], 0), tracks)
    assert torch.equal(torch.cat([a['tracks_visible'], b['tracks_visible']], 0), visible)
    assert torch.equal(b['carry']['track']['points'], tracks[-1]) and torch.equal(b['carry']['track']['alive'], visible[-1])
    with pytest.raises(ValueError, match='track_points'):
        model.forward_sequence(frames[3:], carry=a['carry'], track_points=torch.zeros(5, 2), **args)
    # without the keyword a carry with tracks gives what a carry without gives
    c = model.forward_sequence(frames[3:], carry=a['carry'], **args)
    assert set(c) == {'flow', 'flow_bwd', 'carry'} and 'track' not in c['carry']


def test_sequence_track_points_argument_errors(seq):
    model, kw, frames = seq
    with pytest.raises(ValueError, match='track_points'):
        model.forward_sequence(frames, task='depth', track_points=4, **kw)
    for bad in (0, 2.5, 'sparse', torch.zeros(3, 3), True):
        with pytest.raises(ValueError, match='track_points'):
            model.forward_sequence(frames, track_points=bad, **kw)


# ------------------------------------------------------------------ the frame-directory driver with --track-grid
class ShiftModel:
    """Stands in for the model in ``video.run_directory``: a smooth seeded flow per pair, whatever the frames show."""

    def __init__(self):
        self.pair = 0

    def forward_sequence(self, frames, pred_bidir_flow=False, pairs_per_launch=8, carry=None, **kw):
        pairs = frames.shape[0] - (0 if carry is not None else 1)
        h, w = frames.shape[-2:]
        fwd = torch.cat([tu.smooth_flows(1, h, w, 50 + self.pair + i) for i in range(pairs)], 0)
        self.pair += pairs
        out = {'flow': fwd, 'carry': frames[-1:]}
        if pred_bidir_flow:
            out['flow_bwd'] = tu.backward_flows(fwd, 9)
        return out


@pytest.mark.parametrize('bidir', [False, True])
def test_run_directory_writes_tracks(tmp_path, bidir):
    pytest.importorskip('PIL')
    from unimatch_amd import io
    rng = np.random.default_rng(0)
    (tmp_path / 'in').mkdir()
    for i in range(6):
        io.write_png8(str(tmp_path / 'in' / f'{i:02d}.png'), rng.integers(0, 256, (40, 56, 3), dtype=np.uint8))
    paths = video.list_frames(str(tmp_path / 'in'))
    out = tmp_path / 'out'
    n = video.run_directory(ShiftModel(), paths, str(out), {}, padding_factor=8, pred_bidir_flow=bidir, save_flo=True,
                            pairs_per_launch=2, device='cpu', track_grid=4)
    assert n == 5
    got = np.load(out / 'tracks.npz')
    assert got['tracks'].shape == (5, 10 * 14, 2) and got['visible'].shape == (5, 140) and got['visible'].dtype == np.bool_
    assert np.array_equal(got['start'], video.start_grid(40, 56, 4).numpy())
    fwd = torch.stack([torch.from_numpy(io.read_flo(str(out / f'{i:04d}_pred.flo'))).permute(2, 0, 1) for i in range(5)], 0)
    occ = None
    if bidir:
        bwd = torch.stack([torch.from_numpy(io.read_flo(str(out / f'{i:04d}_pred_bwd.flo'))).permute(2, 0, 1) for i in range(5)], 0)
        occ = video.forward_backward_consistency_check(fwd, bwd)[0]
        assert not os.path.exists(out / '0000_occ_fwd.png')                        # the mask is written with --fwd-bwd-check only
    tracks, visible = video.chain_flows(fwd.contiguous(), occ, stride=4)
    assert np.array_equal(got['tracks'], tracks.numpy()) and np.array_equal(got['visible'], visible.numpy())
    assert visible[-1].any() and not visible[-1].all()
