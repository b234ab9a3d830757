"""The forward-flag matrix (tests/forward_flags.py) without a GPU: the reference's answers pin the oracle, the oracle pins the
product's host path.  What remains unknown after this file is only the GPU leg (tests/test_forward_flags_gpu.py).

Measured when the matrix was written (CONDITIONED weights, outputs of mean magnitude 1 .. 38): oracle fp32 vs the reference 0 .. 4e-6
mean, product with OracleOps vs the oracle at most 9e-7 mean, fp32 vs fp64 arg-max depth: no pixel apart by more than 1e-3."""
import pytest
import torch

from tests import forward_flags as ff
from tests.oracle_ops import OracleOps


@pytest.mark.parametrize('name', ff.RUNNING)
def test_oracle_matches_the_reference(golden, name):
    """``oracle.model.unimatch_forward`` in fp32 against the reference's own fp32 prediction, with the gate of
    test_end_to_end_single_scale: a few times the reference's spread between two summation orders (8 threads vs 1)."""
    case = ff.BY_NAME[name]
    g = golden(case.fixture)
    ref, spread = g[f'{name}.fp32'], float(g[f'{name}.spread'])
    out = ff.oracle(case, torch.float32)
    assert out.shape == ref.shape
    err = (out - ref).abs().mean().item()
    assert err < max(5 * spread, 1e-5), (name, err, spread)


def _distinguishing_calls(case):
    """The backend calls that tell the case's flags apart -> (must be recorded, must not be recorded)."""
    fwd, task = case.fwd, ff.task_of(case)
    must, never = set(), set()
    if task == 'depth':
        must.add('depth_corr_softmax')
        never |= {'local_corr_softmax', 'global_corr_softmax_flow', 'global_corr_softmax_stereo'}
    else:
        radii = fwd['corr_radius_list']
        (must if any(r > 0 for r in radii) else never).add('local_corr_softmax')
        glob = 'global_corr_softmax_flow' if task == 'flow' else 'global_corr_softmax_stereo'
        (must if any(r == -1 for r in radii) else never).add(glob)
    props = fwd['prop_radius_list']
    (must if any(r > 0 for r in props) else never).add('prop_local')
    (must if any(r <= 0 for r in props) else never).add('prop_global')
    (must if case.ctor['reg_refine'] else never).add('local_corr_with_flow')
    return must, never


@pytest.mark.parametrize('name', ff.RUNNING)
def test_product_host_path_matches_the_oracle(name):
    """The product's per-scale loop, stacking, warps, sign conventions and task dispatch with the CPU oracle as backend, against
    ``unimatch_forward`` in fp32: mean abs < 1e-5 (same arithmetic in another order; CONDITIONED weights keep it that close), and the
    backend saw the calls that distinguish the flags."""
    case = ff.BY_NAME[name]
    i0, i1, cam = ff.inputs(case)
    ops = OracleOps()
    model = ff.build_model(case).bind_ops(ops)
    pred = model(i0, i1, **case.fwd, **cam)['flow_preds'][0]
    want = ff.oracle(case, torch.float32)
    assert pred.shape == want.shape
    err = (pred - want).abs().mean().item()
    assert err < 1e-5, (name, err)
    called = {c[0] for c in ops.calls}
    must, never = _distinguishing_calls(case)
    assert must <= called and not (never & called), (name, sorted(called))
    if case.ctor['reg_refine']:
        assert sum(c[0] == 'local_corr_with_flow' for c in ops.calls) == case.fwd['num_reg_refine']


def test_argmax_depth_is_reachable_in_fp32():
    """The GPU leg allows ``depth_s1_argmax`` 1 % of pixels further than 1e-3 from the fp64 oracle (a near-tie flips a candidate and
    the convex upsampling spreads it over a block).  That cap is a condition on the case, not a courtesy: plain fp32 arithmetic meets
    it with NO such pixel.  A seed that breaks this is replaced in the case table."""
    case = ff.BY_NAME['depth_s1_argmax']
    d = (ff.oracle(case, torch.float32).double() - ff.oracle(case, torch.float64)).abs()
    assert (d > 1e-3).sum().item() == 0, d.max().item()


class _Untouchable:
    """A backend whose every attribute access fails the test."""

    def __getattr__(self, attr):
        pytest.fail(f'the backend was touched ({attr}) before the flags were refused')


@pytest.mark.parametrize('name', ff.RAISING)
def test_flags_the_reference_cannot_run_are_refused_up_front(golden, name):
    """``pred_bidir_flow`` on a one-scale model with refinement: the reference fails in a ``view`` (recorded in the fixture) because its
    features are never stacked at scale 0.  The product says so in a ValueError naming the three settings -- before the encoder, before
    any backend call -- from ``forward`` and from ``forward_sequence`` alike."""
    case = ff.BY_NAME[name]
    assert str(golden(case.fixture)._z[f'{name}.raises']) == case.raises
    i0, i1, cam = ff.inputs(case)
    model = ff.build_model(case).bind_ops(_Untouchable())
    for call in (lambda: model(i0, i1, **case.fwd, **cam),
                 lambda: model.forward_sequence(torch.cat([i0, i1], 0), **case.fwd)):
        with pytest.raises(ValueError) as e:
            call()
        assert all(word in str(e.value) for word in ('pred_bidir_flow', 'reg_refine', 'num_scales'))
    # the neighbouring flag sets are not caught by the guard: one direction on this model, both on two scales (flow_s2_rr3_bidir)
    ops = OracleOps()
    ok = model.bind_ops(ops)(i0, i1, **dict(case.fwd, pred_bidir_flow=False))['flow_preds'][0]
    assert ok.shape == (case.batch, 2) + case.size
