"""CPU tests of the multi-view plane sweep: the host restatement's identities in float64 (``confidence.depth_match_logits_multi_host``),
the properties of the shared test inputs, the C ABI's argument checks without a GPU, and ``UniMatch.forward_multiview`` on host tensors
with the CPU oracle injected as hot-path backend."""
import pytest
import torch

from tests import depth_multiview_util as mv
from tests.oracle_ops import OracleOps
from unimatch_amd import UniMatch, _abi, confidence
from unimatch_amd.synth import CONFIGS, synth_camera, synth_frames, synth_state_dict

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _double(case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = (t.double() for t in mv.inputs(case))
    return f0, f1, h, w, cam, cand


# ------------------------------------------------------------------ the restatement
def test_the_inputs_have_the_properties_of_the_issue_table():
    share = mv.check_input_properties()
    print({k: [round(x, 3) for x in v] for k, v in share.items()})


@pytest.mark.parametrize('case', ['A', 'B', 'C', 'D', 'one64'])
def test_one_source_is_the_two_view_restatement_exactly(case):
    f0, f1, h, w, cam, cand = _double(case)
    for s in range(f0.shape[0]):
        want, seen = confidence.depth_match_logits_host(f0[s], f1[s], h, w, cam[s], cand)
        got, in_view, views = confidence.depth_match_logits_multi_host(f0[s:s + 1], f1[s:s + 1], h, w, cam[s:s + 1], cand)
        assert torch.equal(got, want) and torch.equal(in_view, seen) and in_view.dtype == views.dtype == torch.int32
        assert torch.equal(views.sum(1).to(torch.int32), seen) and int(views.max()) <= 1
        a = confidence.depth_match_stats_multi_host(f0[s:s + 1], f1[s:s + 1], h, w, cam[s:s + 1], cand, peak_radius=2)
        e = confidence.depth_match_stats_host(f0[s], f1[s], h, w, cam[s], cand, 2)
        assert all(torch.equal(x, y) for x, y in zip(a, e))


@pytest.mark.parametrize('times', [2, 4])
def test_a_repeated_source_is_exact(times):
    f0, f1, h, w, cam, cand = _double('B')
    one = confidence.depth_match_logits_multi_host(f0[1:2], f1[1:2], h, w, cam[1:2], cand)
    many = confidence.depth_match_logits_multi_host(f0[1:2].repeat(times, 1, 1, 1), f1[1:2].repeat(times, 1, 1, 1), h, w,
                                                    cam[1:2].repeat(times, 1, 1), cand)
    assert torch.equal(many[0], one[0]) and torch.equal(many[1], one[1]) and torch.equal(many[2], times * one[2])


def test_the_order_of_the_sources_does_not_matter():
    f0, f1, h, w, cam, cand = _double('B')
    want = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand)
    for perm in ([1, 2, 0], [2, 1, 0]):
        got = confidence.depth_match_logits_multi_host(f0[perm], f1[perm], h, w, cam[perm], cand)
        assert (got[0] - want[0]).abs().max().item() <= 1e-12 and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_the_rule_is_a_mean_over_the_sources_that_see_the_candidate():
    f0, f1, h, w, cam, cand = _double('A')
    fused, in_view, views = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand)
    each = [confidence.depth_match_logits_visible_host(f0[s], f1[s], h, w, cam[s], cand) for s in range(2)]
    n = each[0][1].int() + each[1][1].int()
    assert torch.equal(views, n) and torch.equal(in_view, (n >= 1).sum(1).int())
    total = each[0][0] * each[0][1] + each[1][0] * each[1][1]
    assert (fused - total / n.clamp(min=1)).abs().max().item() <= 1e-12
    only_one = n == 1                                      # where one source sees the candidate the plain mean halves the logit
    assert (fused - (each[0][0] + each[1][0]) / 2)[only_one].abs().max().item() > 5


def test_use_switches_sources_off_per_sample_and_never_reads_them():
    f0, f1, h, w, cam, cand = _double('A')
    first = confidence.depth_match_logits_multi_host(f0[:1], f1[:1], h, w, cam[:1], cand)
    g0, g1, gcam = f0.clone(), f1.clone(), cam.clone()
    g0[1], g1[1], gcam[1] = float('nan'), float('nan'), float('nan')
    off = confidence.depth_match_logits_multi_host(g0, g1, h, w, gcam, cand, torch.tensor([[1, 1], [0, 0]], dtype=torch.uint8))
    assert all(torch.equal(a, b) for a, b in zip(off, first))
    whole = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand)
    mixed = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand, torch.tensor([[1, 1], [1, 0]], dtype=torch.bool))
    assert torch.equal(mixed[0][0], whole[0][0]) and torch.equal(mixed[0][1], first[0][1]) and torch.equal(mixed[2][1], first[2][1])
    none = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand, torch.zeros(2, 2, dtype=torch.uint8))
    assert bool((none[0] == 0).all()) and bool((none[1] == 0).all())                   # every source off: uniform
    with pytest.raises(ValueError, match='use'):
        confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand, torch.ones(3, 2, dtype=torch.uint8))


def test_depth_match_multi_on_host_tensors_runs_the_restatement():
    f0, f1, h, w, cam, cand = _double('D')
    out, st = confidence.depth_match_multi(f0, f1, h, w, cam, cand, peak_radius=2)
    logits, seen, _ = confidence.depth_match_logits_multi_host(f0, f1, h, w, cam, cand)
    want = confidence.depth_stats_from_prob_host(torch.softmax(logits, 1), cand, seen, 2)
    assert all(torch.equal(a, b) for a, b in zip(st, want)) and torch.equal(out, mv.soft_argmin(logits, cand))
    hard, _ = confidence.depth_match_multi(f0, f1, h, w, cam, cand, from_argmax=True)
    assert torch.equal(hard[:, 0], cand[want.best.long()])
    with pytest.raises(ValueError, match='peak_radius'):
        confidence.depth_match_multi(f0, f1, h, w, cam, cand, peak_radius=-1)
    with pytest.raises(ValueError, match='source-major'):
        confidence.depth_match_multi(f0[0], f1[0], h, w, cam[0], cand)
    with pytest.raises(ValueError):
        confidence.depth_match_multi(f0.repeat(5, 1, 1, 1), f1.repeat(5, 1, 1, 1), h, w, cam.repeat(5, 1, 1), cand)      # 10 sources


# ------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_without_a_gpu():
    lib = _abi.load()
    p = 0x1000                                   # never dereferenced: every call below fails its argument checks first

    def call(f0=p, f1=p, cam=p, use=None, cand=p, out=p, stats=p, index=p, sources=2, batch=2, h=6, w=8, c=128, d=16, argmax=0, radius=1):
        return lib.um_depth_corr_softmax_multi(f0, f1, cam, use, cand, out, stats, index, sources, batch, h, w, c, d, argmax, radius, None)

    def message():
        return lib.um_last_error_string().decode()

    for null in ('f0', 'f1', 'cam', 'cand', 'out'):
        assert call(**{null: None}) < 0 and 'null pointer' in message(), null
    assert call(c=96) < 0 and 'channels=96' in message()
    assert call(d=0) < 0 and 'num_candidates=0' in message()
    assert call(d=129) < 0 and 'num_candidates=129' in message()
    assert call(sources=0) < 0 and 'sources=0' in message()
    assert call(sources=9) < 0 and 'sources=9' in message()
    assert call(radius=-1) < 0 and 'peak_radius=-1' in message()
    assert call(batch=0) < 0 and call(h=0) < 0
    assert lib.um_version() == 220


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


@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_forward_multiview_on_the_host(name):
    model, kw = _model(name)
    kw.pop('task')
    x = _frames(4, 64, 96, 2410)
    k, rel = synth_camera(3, 64, 96)
    ref, nxt, prv = x[1:3], x[2:4], x[0:2]
    pose_next, pose_prev = rel[1:3], torch.inverse(rel[0:2])
    plain = model(ref, nxt, task='depth', intrinsics=k[1:3], pose=pose_next, **kw)['flow_preds'][0]
    one = model.forward_multiview(ref, nxt[:, None], intrinsics=k[1:3], poses=pose_next[:, None], **kw)
    assert set(one) == {'flow_preds'} and torch.equal(one['flow_preds'][0], plain)          # S = 1 is forward
    srcs, poses = torch.stack([nxt, prv], 1), torch.stack([pose_next, pose_prev], 1)
    model.debug_taps = taps = {}
    two = model.forward_multiview(ref, srcs, intrinsics=k[1:3], poses=poses, return_confidence=True, peak_radius=2, **kw)
    model.debug_taps = None
    depth = two['flow_preds'][0]
    assert tuple(depth.shape) == (2, 64, 96) and bool(torch.isfinite(depth).all())
    lo, hi = 1. / kw.get('min_depth', 1. / 0.5), 1. / kw.get('max_depth', 1. / 10)
    assert depth.min().item() >= min(lo, hi) * (1 - 1e-6) and depth.max().item() <= max(lo, hi) * (1 + 1e-6)
    assert (depth - plain).abs().max().item() > 1e-3 * max(1.0, plain.abs().max().item())     # the second view has a say
    # the confidence is that of the fused distribution of the tapped tokens
    conf = two['depth_confidence']
    assert set(conf) == {'max_prob', 'entropy', 'variance', 'peak_mass', 'best', 'in_view', 'scale', 'num_candidates'}
    tok0, tok1 = (taps[n].flatten(2).transpose(1, 2).contiguous() for n in ('f0_s0', 'f1_s0'))
    assert tok0.shape[0] == 4                                                               # B S pairs in one stream
    kf = k[1:3].clone()
    kf[:, :2] = kf[:, :2] / 8
    pose_all = poses.transpose(0, 1).reshape(4, 4, 4)
    kk = kf.repeat(2, 1, 1)
    cam = torch.cat([torch.inverse(kk).flatten(1), pose_all[:, :3, :3].flatten(1), pose_all[:, :3, 3], kk.flatten(1)], 1).float()
    cand = torch.linspace(kw.get('min_depth', 1. / 0.5), kw.get('max_depth', 1. / 10), kw.get('num_depth_candidates', 64)).float()
    want = confidence.depth_match_stats_multi_host(tok0.view(2, 2, 96, 128), tok1.view(2, 2, 96, 128), 8, 12, cam.view(2, 2, 30), cand,
                                                   peak_radius=2)
    for key in ('max_prob', 'entropy', 'variance', 'peak_mass', 'best', 'in_view'):
        assert tuple(conf[key].shape) == (2, 8, 12) and torch.equal(conf[key], getattr(want, key)), key
    assert conf['scale'] == 8 and conf['num_candidates'] == 64


def test_forward_multiview_refusals():
    model, kw = _model('gmdepth_s1')
    kw.pop('task')
    x = _frames(3, 64, 96, 2411)
    k, rel = synth_camera(2, 64, 96)
    args = dict(intrinsics=k[:1], poses=rel[:1, None], **kw)
    with pytest.raises(ValueError, match='pred_bidir_depth'):
        model.forward_multiview(x[:1], x[1:2, None], pred_bidir_depth=True, **args)
    with pytest.raises(ValueError, match="task='depth'"):
        model.forward_multiview(x[:1], x[1:2, None], task='flow', **args)
    with pytest.raises(ValueError, match='img_srcs'):
        model.forward_multiview(x[:1], x[1:2], **args)
    with pytest.raises(ValueError, match='poses'):
        model.forward_multiview(x[:1], x[1:2, None], intrinsics=k[:1], poses=rel[:1], **kw)
    with pytest.raises(ValueError, match='peak_radius'):
        model.forward_multiview(x[:1], x[1:2, None], return_confidence=True, peak_radius=-1, **args)
    two_scales, _ = _model('gmflow_s2_rr6')
    with pytest.raises(ValueError, match='one-scale'):
        two_scales.forward_multiview(x[:1], x[1:2, None], intrinsics=k[:1], poses=rel[:1, None], attn_splits_list=[2], prop_radius_list=[-1])
