"""GPU tests of the point tracks: ``um_flow_chain`` (through ``video.chain_flows``) against the fp64 restatement and the reference's
composition of flows, its determinism and statelessness, and ``UniMatch.forward_sequence(track_points=...)``."""
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, video
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_frames, synth_state_dict
from tests import tracks_util as tu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tracks.npz')


def dev(t):
    return None if t is None else t.to(DEV)


def run(fwd, occ, **kw):
    tracks, visible = video.chain_flows(dev(fwd), dev(occ), **{k: dev(v) if torch.is_tensor(v) else v for k, v in kw.items()})
    assert tracks.is_cuda and tracks.dtype == torch.float32 and visible.is_cuda and visible.dtype == torch.bool
    return tracks, visible


@pytest.mark.parametrize('case', tu.CASES, ids=lambda c: 'x'.join(map(str, c[:3])))
def test_kernel_dense_against_fp64(case):
    fwd, occ = tu.inputs(*case)
    worst = tu.accept(*run(fwd, occ), tu.chain_fp64(fwd, occ))
    # one pair (P = 1): the first of the case
    one = None if occ is None else occ[:1]
    first = tu.accept(*run(fwd[:1], one), tu.chain_fp64(fwd[:1], one))
    print(f'um_flow_chain dense {case[:3]}: max |d| {worst:.3e} px (first pair alone {first:.3e})')
    # the start grid is the documented one
    tracks, _ = run(torch.zeros_like(fwd[:1]), None)
    assert torch.equal(tracks[0].cpu(), video.start_grid(*fwd.shape[2:]))


def test_kernel_stride_grid_against_fp64():
    fwd, occ = tu.inputs(8, 33, 47, 3)
    tracks, visible = run(fwd, occ, stride=3)
    assert tuple(tracks.shape) == (8, 11 * 16, 2)
    worst = tu.accept(tracks, visible, tu.chain_fp64(fwd, occ, stride=3))
    print(f'um_flow_chain stride 3 at 33x47: max |d| {worst:.3e} px')
    zero, _ = run(torch.zeros_like(fwd[:1]), None, stride=3)
    assert torch.equal(zero[0].cpu(), video.start_grid(33, 47, 3))


def test_kernel_sparse_points_against_fp64():
    fwd, occ = tu.inputs(6, 64, 97, 4)
    pts, dead = tu.sparse_points(64, 97)
    tracks, visible = run(fwd, occ, points=pts)
    worst = tu.accept(tracks, visible, tu.chain_fp64(fwd, occ, points=pts))
    print(f'um_flow_chain 257 sparse points at 64x97: max |d| {worst:.3e} px')
    tracks, visible = tracks.cpu(), visible.cpu()
    assert not visible[:, dead].any()
    frozen = torch.nan_to_num(pts[dead], nan=7.0, posinf=8.0)
    assert all(torch.equal(torch.nan_to_num(row[dead], nan=7.0, posinf=8.0), frozen) for row in tracks)
    off = torch.ones(257, dtype=torch.bool)
    off[100:120] = False
    t2, v2 = run(fwd, occ, points=pts, alive=off)
    assert not v2[:, 100:120].any() and torch.equal(t2[-1, 100:120].cpu(), pts[100:120])
    # a flow far out of frame, inf and NaN: the tracks die where they are, nothing is read out of bounds
    wild = fwd.clone()
    wild[0, 0, :, :30] = 3e9
    wild[0, 1, :20, 30:60] = float('nan')
    wild[1, 0, :, 60:] = float('-inf')
    tracks, visible = (t.cpu() for t in run(wild, None))
    t64, v64, margin = tu.chain_fp64(wild, None)
    agree = (visible == v64).all(0)
    assert (margin[~agree] < tu.MARGIN_TOL).all() and agree.float().mean() > 0.99
    finite = torch.isfinite(t64)
    assert torch.equal(torch.isfinite(tracks)[:, agree], finite[:, agree])
    both = finite & agree[None, :, None]
    err = (tracks.double() - t64).abs()[both]
    assert (err <= tu.POS_TOL + 1e-6 * t64[both].abs()).all()           # 3e9 + x rounds to float32's spacing there
    assert (~visible[0]).sum() >= 30 * 64 and visible[-1].any()


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_kernel_matches_reference_composition(tag):
    golden = np.load(GOLDEN)
    fwd, comp = torch.from_numpy(golden[f'fwd_{tag}']), torch.from_numpy(golden[f'comp_{tag}'])
    tracks, visible = run(fwd, None)
    tu.check_composition(tracks, visible, comp, *fwd.shape[2:])


def test_kernel_is_deterministic_and_stateless():
    fwd, occ = (dev(t) for t in tu.inputs(8, 33, 47, 3))
    other = tuple(dev(t) for t in tu.inputs(6, 64, 97, 4))
    first = video.chain_flows(fwd, occ)
    again = [video.chain_flows(fwd, occ) for _ in range(2)]
    video.chain_flows(*other, stride=2)
    after = video.chain_flows(fwd, occ)
    t3, v3 = video.chain_flows(fwd[:3], occ[:3])
    t5, v5 = video.chain_flows(fwd[3:], occ[3:], points=t3[-1], alive=v3[-1])
    torch.cuda.synchronize()
    for t, v in again + [after, (torch.cat([t3, t5], 0), torch.cat([v3, v5], 0))]:
        assert torch.equal(t, first[0]) and torch.equal(v, first[1])
    assert first[1][-1].any() and not first[1][-1].all()


def test_forward_sequence_tracks():
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    frames = synth_frames(6, 128, 192).to(DEV)
    args = dict(pairs_per_launch=4, pred_bidir_flow=True, **kw)
    plain = model.forward_sequence(frames, consistency_check=True, **args)
    assert set(plain) == {'flow', 'flow_bwd', 'occ_fwd', 'occ_bwd', 'carry'} and set(plain['carry']) == {'features', 'frame', 'state'}
    out = model.forward_sequence(frames, consistency_check=True, track_points=16, **args)
    assert set(out) == set(plain) | {'tracks', 'tracks_visible'} and set(out['carry']) == {'features', 'frame', 'state', 'track'}
    for key in ('flow', 'flow_bwd', 'occ_fwd', 'occ_bwd'):
        assert torch.equal(out[key], plain[key]), key
    assert tuple(out['tracks'].shape) == (5, 8 * 12, 2) and out['tracks_visible'].dtype == torch.bool
    tracks, visible = video.chain_flows(out['flow'], out['occ_fwd'], stride=16)
    assert torch.equal(out['tracks'], tracks) and torch.equal(out['tracks_visible'], visible)
    # without consistency_check the same mask is used and not returned
    quiet = model.forward_sequence(frames, track_points=16, **args)
    assert set(quiet) == {'flow', 'flow_bwd', 'tracks', 'tracks_visible', 'carry'}
    assert torch.equal(quiet['tracks'], tracks) and torch.equal(quiet['tracks_visible'], visible)
    # fed in pieces with the carry: chunks of 4 and 1 pairs, as in the one call
    a = model.forward_sequence(frames[:5], track_points=16, **args)
    b = model.forward_sequence(frames[5:], carry=a['carry'], track_points=16, **args)
    assert torch.equal(torch.cat([a['tracks'], b['tracks']], 0), tracks)
    assert torch.equal(torch.cat([a['tracks_visible'], b['tracks_visible']], 0), visible)
    # frame bounds only without the backward flow
    fwd_only = model.forward_sequence(frames, pairs_per_launch=4, track_points=16, **kw)
    t2, v2 = video.chain_flows(fwd_only['flow'], None, stride=16)
    assert torch.equal(fwd_only['tracks'], t2) and torch.equal(fwd_only['tracks_visible'], v2)
    model.check_operand_range()
