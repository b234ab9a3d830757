"""The forward-flag matrix (tests/forward_flags.py) on the GPU: ``UniMatch.forward`` with ``HipOps`` in exact mode against the CPU oracle
in fp64, for the flag sets whose branches of ``_match`` and ``NhwcUpdateBlock`` exist only on the device (``stream=both`` vs separate
token streams, the bidirectional stacking at ``s > 0``, ``flow_warp`` / ``flow_upsample2x``, ``depth_cam`` / ``rigid_flow``, ``pred_out``,
the hoisted gates at batch 2B).  The CPU leg (tests/test_forward_flags_cpu.py) pins the oracle to the reference on the same cases.

Gates, PER SAMPLE (a swapped or half-written sample cannot hide in a batch mean), with ``e32`` the fp32 oracle's error against fp64:

* mean: ``mean|pred - fp64| <= 3 * mean(e32) + 1e-4`` -- the project's end-to-end gate (test_end_to_end_exact_mode), unchanged;
* maximum: ``max|pred - fp64| <= 3 * max(e32) + MAX_FLOOR``.  ``MAX_FLOOR`` is 4 x the largest per-sample maximum error the exact mode
  showed over the whole matrix when it was first run (``profiles/forward_flags.txt``, written by ``tools/forward_flags_table.py``),
  and never more than the 1e-3 EPE gate in the prediction's own unit;
* ``depth_s1_argmax``: a near-tie flips a candidate and the convex upsampling spreads the flip over a block, so the two gates are
  replaced by a cap -- at most 1 % of pixels further than 1e-3 from fp64 (the fp32 oracle has none: test_argmax_depth_is_reachable_in_fp32)
  -- and the mean gate on the other pixels.
"""
import pytest
import torch

from tests import forward_flags as ff
from unimatch_amd.ops import KernelTimer

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# 4 x 5.08e-5, the largest per-sample max|pred - fp64| of profiles/forward_flags.txt (stereo_s2: disparities of ~34 px, where the fp32
# oracle's own worst pixel is 5.09e-5); every other row of the table is below 4.6e-5
MAX_FLOOR = 2.0e-4
assert MAX_FLOOR <= 1e-3
ARGMAX_CAP, ARGMAX_TOL = 0.01, 1e-3


def run_gpu(case, parts=1, timer=False, calls=1, images=None):
    """``calls`` forwards of the case in exact mode on one model -> (predictions on the CPU, {kernel name: launches} of all calls or
    None).  ``parts``: the value of ``launch_parts`` (1: one forward of the whole batch).  ``images``: ``(img0, img1)`` in place of
    the case's own pair (tests/degenerate_content.py)."""
    model = ff.build_model(case).to(DEV).set_precision('exact')
    i0, i1, cam = ff.inputs(case)
    if images is not None:
        i0, i1 = images
    i0, i1, cam = i0.to(DEV), i1.to(DEV), {k: v.to(DEV) for k, v in cam.items()}
    model.launch_parts = parts
    if timer:
        model.ops.timer = KernelTimer()
    preds = [model(i0, i1, **case.fwd, **cam)['flow_preds'][0] for _ in range(calls)]
    model.check_operand_range()
    launches = {k: v['calls'] for k, v in model.ops.timer.summary().items()} if timer else None
    return [p.cpu() for p in preds], launches


def _answers(case, answers):
    """The (fp64, fp32) oracle answers the gates compare with: the case's own, or the pair handed in for other images."""
    return answers if answers is not None else (ff.oracle(case, torch.float64), ff.oracle(case, torch.float32))


def sample_errors(case, pred, answers=None):
    """Per sample: (mean, max) of |pred - fp64| and of |fp32 oracle - fp64|, as ``[(gpu_mean, gpu_max, f32_mean, f32_max), ...]``."""
    truth, f32 = _answers(case, answers)
    assert pred.shape == truth.shape, (case.name, tuple(pred.shape), tuple(truth.shape))
    out = []
    for n in range(truth.shape[0]):
        d, d32 = (pred[n].double() - truth[n]).abs(), (f32[n].double() - truth[n]).abs()
        out.append((d.mean().item(), d.max().item(), d32.mean().item(), d32.max().item()))
    return out


def check_gates(case, pred, answers=None, tag=''):
    """The module's gates on one prediction; ``answers``: the (fp64, fp32) oracle answers when the images are not the case's own."""
    assert torch.isfinite(pred).all(), case.name
    truth, f32 = _answers(case, answers)
    figures = sample_errors(case, pred, answers)
    print(case.name + tag, ' '.join(f'[{a:.2e} {b:.2e} | {c:.2e} {d:.2e}]' for a, b, c, d in figures))
    for n, (g_mean, g_max, f_mean, f_max) in enumerate(figures):
        if case.fwd.get('depth_from_argmax'):
            d = (pred[n].double() - truth[n]).abs()
            far = d > ARGMAX_TOL
            assert far.float().mean().item() <= ARGMAX_CAP, (case.name, n, far.float().mean().item())
            near32 = (f32[n].double() - truth[n]).abs()[~far]
            assert d[~far].mean().item() <= 3 * near32.mean().item() + 1e-4, (case.name, n, d[~far].mean().item())
            continue
        assert g_mean <= 3 * f_mean + 1e-4, (case.name, n, 'mean', g_mean, f_mean)
        assert g_max <= 3 * f_max + MAX_FLOOR, (case.name, n, 'max', g_max, f_max)


def expected_launches(case):
    """The ``KernelTimer`` names that distinguish the case -> ({name: exact count or None for 'at least once'}, names that must not
    appear).  Names as ``HipOps`` records them: global_corr_flow / global_corr_stereo / local_corr_softmax / depth_corr_softmax for
    the matching layer, prop_global / prop_local, local_corr_with_flow once per refinement iteration."""
    fwd, task = case.fwd, ff.task_of(case)
    must, never = {}, set()

    def want(name, present):
        if present:
            must[name] = None
        else:
            never.add(name)
    if task == 'depth':
        must['depth_corr_softmax'] = 1
        never |= {'global_corr_flow', 'global_corr_stereo', 'local_corr_softmax'}
    else:
        radii = fwd['corr_radius_list']
        want('local_corr_softmax', any(r > 0 for r in radii))
        want('global_corr_flow', task == 'flow' and -1 in radii)
        want('global_corr_stereo', task == 'stereo' and -1 in radii)
        never.add('depth_corr_softmax')
    props = fwd['prop_radius_list']
    want('prop_local', any(r > 0 for r in props))
    want('prop_global', any(r <= 0 for r in props))
    if case.ctor['reg_refine']:
        must['local_corr_with_flow'] = fwd['num_reg_refine']
    else:
        never.add('local_corr_with_flow')
    return must, never


@pytest.mark.parametrize('name', ff.RUNNING)
def test_forward_flags_against_fp64(name):
    """One forward per flag set against the fp64 oracle under the module's gates, and the launches that distinguish the flag set ran
    (and the ones of the neighbouring flag set did not)."""
    case = ff.BY_NAME[name]
    (pred,), launches = run_gpu(case, timer=True)
    must, never = expected_launches(case)
    for kernel, count in must.items():
        assert kernel in launches and (count is None or launches[kernel] == count), (name, kernel, launches.get(kernel))
    assert not (never & set(launches)), (name, sorted(never & set(launches)))
    check_gates(case, pred)


@pytest.mark.parametrize('name', ['flow_s2_rr2_b2', 'stereo_s2_rr2_b2'])
def test_forward_flags_as_two_concurrent_parts(name):
    """The batch-2 refinement cases once more as two half-batch forwards on two streams (``launch_parts = 2``, as
    test_two_parts_with_bidirectional_flow_keep_the_reference_layout forces it): the first call runs the parts one after the other,
    the second one concurrently; both give the same bits and pass the same gates, sample by sample."""
    case = ff.BY_NAME[name]
    (first, second), _ = run_gpu(case, parts=2, calls=2)
    assert torch.equal(first, second), (name, (first - second).abs().max().item())
    check_gates(case, second)


@pytest.mark.parametrize('name', ff.RAISING)
def test_refused_flags_launch_nothing(name):
    """``pred_bidir_flow`` on one scale with refinement is refused with a ValueError before the encoder: the launch census counts no
    kernel.  (Unrefused, the refinement block would run at batch 2B on B feature samples.)"""
    from unimatch_amd import _abi
    case = ff.BY_NAME[name]
    model = ff.build_model(case).to(DEV).set_precision('exact')
    assert model.ops is not None                                   # the backend exists before the census starts
    i0, i1, _ = ff.inputs(case)
    i0, i1 = i0.to(DEV), i1.to(DEV)
    lib = _abi.load()
    lib.um_census_enable(1)
    try:
        with pytest.raises(ValueError, match='pred_bidir_flow'):
            model(i0, i1, **case.fwd)
        with pytest.raises(ValueError, match='pred_bidir_flow'):
            model.forward_sequence(torch.cat([i0, i1], 0), **case.fwd)
        census = _abi.census(lib)
    finally:
        lib.um_census_enable(0)
    assert not any(census.values()), census
