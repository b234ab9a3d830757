"""Pin the CPU oracle (oracle/) to the real reference through the committed golden fixtures.

Every fixture in tests/golden/*.npz was produced by executing /root/reference (tests/golden/make_golden.py).
Tolerances are fp32 re-association noise: the oracle evaluates the same maths with index arithmetic instead
of roll/split/mask/grid_sample tensors.
"""
import pytest
import torch

from oracle import hotpath as hp
from oracle import model as om
from unimatch_amd.synth import CONFIGS, synth_camera, synth_images, synth_state_dict
from unimatch_amd import UniMatch

C = 128


def maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


def test_position_table_is_bit_exact(golden):
    g = golden('position')
    for (h, w) in ((4, 6), (8, 12), (16, 24)):
        assert torch.equal(hp.position_table(h, w, C), g[f'pos_{h}x{w}'])
    for k, tag in ((2, 'k2'), (1, 'k1')):
        a0, a1 = hp.add_position(g['f0'], g['f1'], k)
        assert torch.equal(a0, g[f'add_{tag}_0']) and torch.equal(a1, g[f'add_{tag}_1'])


def _attn_geometry(tag, h, w, k, shift):
    if tag.startswith('win2d'):
        return (h // k, w // k, (h // k // 2) if shift else 0, (w // k // 2) if shift else 0)
    if tag.startswith('winrow'):
        return (1, w // k, 0, (w // k // 2) if shift else 0)
    if tag.startswith('row'):
        return (1, w, 0, 0)
    return (h, w, 0, 0)


def attention_cases(g):
    return sorted({k.split('.')[0] for k in g.keys()})


def test_window_attention(golden):
    g = golden('attention')
    cases = attention_cases(g)
    assert len(cases) == 10
    for tag in cases:
        h, w, k, shift = (int(x) for x in g[f'{tag}.meta'])
        geom = _attn_geometry(tag, h, w, k, shift)
        out = hp.window_attention(g[f'{tag}.q'], g[f'{tag}.k'], g[f'{tag}.v'], h, w, *geom)
        assert maxdiff(out, g[f'{tag}.out']) < 2e-5, tag


def test_attention_geometry_dispatch():
    assert hp.attention_geometry('swin', True, 2, 8, 12, True) == (4, 6, 2, 3)
    assert hp.attention_geometry('swin', False, 2, 8, 12, False) == (4, 6, 0, 0)
    assert hp.attention_geometry('swin', True, 1, 8, 12, True) == (8, 12, 0, 0)
    assert hp.attention_geometry('self_swin2d_cross_1d', False, 2, 8, 12, True) == (1, 12, 0, 0)
    assert hp.attention_geometry('self_swin2d_cross_swin1d', False, 4, 8, 16, True) == (1, 4, 0, 2)
    assert hp.attention_geometry('self_swin2d_cross_swin1d', True, 4, 8, 16, True) == (2, 4, 1, 2)
    assert hp.attention_geometry('self_swin2d_cross_swin1d', False, 1, 8, 16, True) == (1, 16, 0, 0)
    assert hp.attention_geometry(None or '', True, 2, 8, 12, True) == (8, 12, 0, 0)


def test_feature_transformer(golden):
    g = golden('transformer')
    proto = UniMatch().transformer
    sd = synth_state_dict({k: v.shape for k, v in proto.state_dict().items()}, seed=7)
    for attn_type, k in (('swin', 2), ('swin', 1), ('self_swin2d_cross_1d', 2),
                         ('self_swin2d_cross_swin1d', 2), ('self_swin2d_cross_swin1d', 4)):
        tag = f'{attn_type}_k{k}'
        o0, o1 = hp.feature_transformer(g[f'{tag}.f0'], g[f'{tag}.f1'], sd, attn_type, k)
        assert maxdiff(o0, g[f'{tag}.o0']) < 2e-4, tag
        assert maxdiff(o1, g[f'{tag}.o1']) < 2e-4, tag


@pytest.mark.parametrize('tag', ['soft', 'peaky'])
def test_matching_layers(golden, tag):
    g = golden('matching')
    f0, f1 = g[f'{tag}.f0'], g[f'{tag}.f1']
    tol = 2e-4
    assert maxdiff(hp.global_corr_softmax_flow(f0, f1, False), g[f'{tag}.global_flow']) < tol
    assert maxdiff(hp.global_corr_softmax_flow(f0, f1, True), g[f'{tag}.global_flow_bidir']) < tol
    assert maxdiff(hp.local_corr_softmax(f0, f1, 4), g[f'{tag}.local_flow_r4']) < tol
    assert maxdiff(hp.local_corr_softmax(f0, f1, 2), g[f'{tag}.local_flow_r2']) < tol
    assert maxdiff(hp.global_corr_softmax_stereo(f0, f1), g[f'{tag}.stereo_global']) < tol
    assert maxdiff(hp.local_corr_softmax(f0, f1, 4, one_d=True), g[f'{tag}.stereo_local_r4']) < tol
    flow = g[f'{tag}.flow_in']
    assert maxdiff(hp.local_corr_with_flow(f0, f1, flow, 4), g[f'{tag}.cost_r4']) < tol
    assert maxdiff(hp.local_corr_with_flow(f0, f1, flow, 2), g[f'{tag}.cost_r2']) < tol
    k, pose, cand = g[f'{tag}.K'], g[f'{tag}.pose'], g[f'{tag}.cand']
    assert maxdiff(hp.depth_corr_softmax(f0, f1, k, pose, cand), g[f'{tag}.depth']) < tol
    assert maxdiff(hp.depth_corr_softmax(f0, f1, k, pose, cand, bidir=True), g[f'{tag}.depth_bidir']) < tol
    am = hp.depth_corr_softmax(f0, f1, k, pose, cand, from_argmax=True)
    assert (am - g[f'{tag}.depth_argmax']).abs().gt(1e-6).float().mean().item() < 0.01   # argmax ties only


def test_propagation(golden):
    g = golden('propagation')
    proto = UniMatch().feature_flow_attn
    sd = {'feature_flow_attn.' + k: v for k, v in
          synth_state_dict({k: v.shape for k, v in proto.state_dict().items()}, seed=11).items()}
    f0 = g['f0']
    for vch in (2, 1):
        val = g[f'val{vch}']
        assert maxdiff(hp.prop_global(f0, val, sd), g[f'global{vch}']) < 1e-4
        assert maxdiff(hp.prop_local(f0, val, sd, 1), g[f'local{vch}_r1']) < 1e-4
        assert maxdiff(hp.prop_local(f0, val, sd, 2), g[f'local{vch}_r2']) < 1e-4


E2E = {'gmflow_s1': (64, 96), 'gmstereo_s1': (64, 96), 'gmdepth_s1': (96, 128), 'gmdepth_s1_rr1': (96, 128),
       'gmflow_s2_rr6': (128, 192), 'gmstereo_s2_rr3': (128, 192)}


def oracle_e2e(name, dtype=torch.float32, extra=None):
    ck, fk = CONFIGS[name]
    hh, ww = E2E[name]
    sd = synth_state_dict({k: v.shape for k, v in UniMatch(**ck).state_dict().items()}, refine_gain=0.02)
    i0, i1 = synth_images(1, hh, ww, seed=1000, kind='shift', normalized=(fk['task'] != 'flow'))
    kw = {k: v for k, v in fk.items()}
    kw.update(num_scales=ck['num_scales'], upsample_factor=ck['upsample_factor'], reg_refine=ck['reg_refine'])
    if extra:
        kw.update(extra)
    if fk['task'] == 'depth':
        k, pose = synth_camera(1, hh, ww)
        kw.update(intrinsics=k.to(dtype), pose=pose.to(dtype))
    return om.unimatch_forward(sd, i0.to(dtype), i1.to(dtype), **kw)


@pytest.mark.parametrize('name', ['gmflow_s1', 'gmstereo_s1', 'gmdepth_s1', 'gmdepth_s1_rr1'])
def test_end_to_end_single_scale(golden, name):
    """Whole forward vs the reference.  Tolerance = a few times the reference's own fp32 spread between
    two summation orders (8 threads vs 1 thread), which the fixture records."""
    g = golden('e2e')
    ref, ref1 = g[f'{name}.fp32'], g[f'{name}.fp32_1thread']
    out = oracle_e2e(name)
    noise = (ref - ref1).abs().mean().item()
    err = (out - ref).abs().mean().item()
    assert out.shape == ref.shape
    assert err < max(5 * noise, 1e-5), (err, noise)


@pytest.mark.parametrize('name', ['gmflow_s2_rr6', 'gmstereo_s2_rr3'])
def test_end_to_end_two_scale_refine(golden, name):
    """Two-scale + refinement configs are ill-conditioned at random init even with the tamed flow head:
    the reference's own 8-thread vs 1-thread outputs differ at the 1e-1 px level.  The oracle must sit
    inside a few times that spread (stage-level fixtures pin every layer tightly)."""
    g = golden('e2e')
    ref, ref1 = g[f'{name}.fp32'], g[f'{name}.fp32_1thread']
    out = oracle_e2e(name)
    noise = (ref - ref1).abs().mean().item()
    err = (out - ref).abs().mean().item()
    assert out.shape == ref.shape
    assert err < 5 * noise + 1e-3, (err, noise)


def test_end_to_end_bidirectional(golden):
    g = golden('e2e')
    out = oracle_e2e('gmflow_s1', extra=dict(pred_bidir_flow=True))
    assert out.shape == g['gmflow_s1_bidir.fp32'].shape
    assert (out - g['gmflow_s1_bidir.fp32']).abs().mean().item() < 1e-3
    out = oracle_e2e('gmdepth_s1', extra=dict(pred_bidir_depth=True))
    assert out.shape == g['gmdepth_s1_bidir.fp32'].shape
    assert (out - g['gmdepth_s1_bidir.fp32']).abs().mean().item() < 1e-4


@pytest.mark.parametrize('dilation', [1, 2, 3])
def test_cost_volume_dilation_against_the_reference(golden, dilation):
    """The oracle's dilated cost volume (the checker of um_local_corr_with_flow_dilated) against the real
    local_correlation_with_flow(..., dilation=d) (matching.py:86-123) -- no caller of the reference uses dilation != 1, so its
    output for d = 1, 2, 3 on seeded inputs is a fixture of its own (tests/golden/dilation.npz)."""
    g = golden('dilation')
    f0, f1, flow = g['f0'], g['f1'], g['flow']
    want = g[f'dilation{dilation}']
    assert maxdiff(hp.local_corr_with_flow_dilated(f0, f1, flow, 4, dilation), want) < 2e-5
    if dilation == 1:
        assert maxdiff(hp.local_corr_with_flow(f0, f1, flow, 4), want) < 2e-5
