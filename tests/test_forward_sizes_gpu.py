"""The forward-size matrix (tests/forward_sizes.py) on the GPU: ``UniMatch.forward`` with ``HipOps`` in exact mode at sizes whose host
rules no other whole-model test reaches -- the row-window and generic convolutions inside the encoder, windows with odd sides and
rounded shifts, windows of two query tiles, 1-D windows of odd length, portrait maps, token counts that are no multiple of 32, maps
below one tile of every kernel -- against the CPU oracle in fp64.  The CPU leg (tests/test_forward_sizes_cpu.py) pins the oracle to the
reference on the same rows and asserts what the matrix reaches.

Gates: ``run_gpu``, ``sample_errors`` and ``check_gates`` of tests/test_forward_flags_gpu.py as they are, per sample (``MAX_FLOOR`` is
that module's number, not measured again here).  Beyond the gates: the launch census shows the kernels the host mirrors predict, two
runs give the same bits, and a model that changes geometry between calls answers as a fresh model does.
"""
import functools

import pytest
import torch

from tests import dispatch_boundaries as db
from tests import forward_flags as ff
from tests import forward_sizes as fs
from tests import test_forward_flags_gpu as flags_gpu
from unimatch_amd import _abi

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CONV_SIDES = ('conv_patch', 'conv_patch_norm', 'conv_rows', 'conv_generic')


def census(lib, fn):
    """fn() with the launch census on -> (result, {variant: launches})."""
    lib.um_census_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        counts = _abi.census(lib)
    finally:
        lib.um_census_enable(0)
    return out, counts


@functools.lru_cache(maxsize=None)
def row(name):
    """Two forwards of the row on one model (``run_gpu``: exact mode, ``check_operand_range`` after them) under the launch census ->
    (the two predictions, the census of ONE forward).  Computed once per process; the tests below look at different sides of it."""
    case = fs.BY_NAME[name]
    (preds, _), counts = census(_abi.load(), lambda: flags_gpu.run_gpu(case, calls=2))
    assert all(v % 2 == 0 for v in counts.values()), (name, 'the two forwards took different kernels', counts)
    return preds, {k: v // 2 for k, v in counts.items()}


@pytest.mark.parametrize('name', fs.RUNNING)
def test_forward_sizes_against_fp64(name):
    """One forward per row against the fp64 oracle under the flag matrix's gates, per sample."""
    case = fs.BY_NAME[name]
    preds, _ = row(name)
    flags_gpu.check_gates(case, preds[0], answers=fs.answers(case))


@pytest.mark.parametrize('name', fs.RUNNING)
def test_two_runs_give_equal_bits(name):
    first, second = row(name)[0]
    assert torch.equal(first, second), (name, (first - second).abs().max().item())


@pytest.mark.parametrize('name', fs.RUNNING)
def test_encoder_runs_the_predicted_convolutions(name):
    """``UniMatch._encode`` alone on the row's images under the launch census: patch, on-load patch, row-window and generic launches
    are those ``db.conv_kind`` gives over the encoder's own layer table (``fs.encoder_convs``)."""
    case = fs.BY_NAME[name]
    model = ff.build_model(case).to(DEV).set_precision('exact')
    assert model.ops is not None
    i0, i1, _ = ff.inputs(case)
    i0, i1 = i0.to(DEV), i1.to(DEV)
    with torch.no_grad():
        feats, counts = census(_abi.load(), lambda: model._encode((i0, i1), ff.task_of(case)))
    assert [tuple(f.shape[-2:]) for f in feats] == fs.maps(case.size, case.ctor['num_scales'])
    want = fs.encoder_census(case.size, case.ctor['num_scales'])
    got = {k: counts[k] for k in CONV_SIDES}
    print('SIZES | encoder |', name, '|', ' '.join(f'{n}:{k}{"+norm" if nl else ""}' for n, _, _, k, nl in
                                                  fs.encoder_convs(case.size, case.ctor['num_scales'])), '|', got)
    assert got == want, (name, got, want)
    assert sum(v for k, v in counts.items() if k not in CONV_SIDES) == 0, counts        # the encoder launches nothing else the census names


@pytest.mark.parametrize('name', fs.RUNNING)
def test_forward_takes_the_planned_sides(name):
    """The sides of a whole forward -- whole-tile or key-split attention, tile or hidden-split FFN, gsv3 / gsv4, the matrix-core or
    VALU cost volumes -- are those the exported plan functions give for the row's geometry on THIS device (``um_window_attn_plan``,
    ``um_ffn_split_workspace_bytes``, ``um_local_corr_with_flow_feat_supported``; gsv: launch_gsv's rule with the device's CU count)."""
    case = fs.BY_NAME[name]
    lib = _abi.load()
    _, counts = row(name)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    attn = {'wattn_tile': 0, 'wattn_ksplit': 0}
    for streams, h, w, wh, ww in fs.attention_launches(case):
        _, split, _ = db.attn_plan(lib, streams, h, w, wh, ww)
        attn['wattn_ksplit' if split else 'wattn_tile'] += 1
    ffn = {'ffn_tile': 0, 'ffn_hsplit': 0}
    for m in fs.ffn_launches(case):
        ffn['ffn_hsplit' if db.ffn_split(lib, m, 1024) > 1 else 'ffn_tile'] += 1
    rest = fs.matching_sides(case, cus, lib.um_local_corr_with_flow_feat_supported)
    print('SIZES | sides |', name, '|', {k: v for k, v in counts.items() if v and k not in CONV_SIDES}, '| CUs', cus)
    for k, v in attn.items():
        assert counts[k] == v, (name, k, counts[k], attn)
    for k, v in ffn.items():
        assert (counts[k] > 0) == (v > 0), (name, k, counts[k], ffn)
    for k, v in rest.items():
        assert (counts[k] > 0) if v is None else (counts[k] == v), (name, k, counts[k], rest)


def _flow_s2rr(size):
    return fs.BY_NAME['flow_s2rr_96x160_b2']._replace(name='flow_s2rr_%dx%d' % size, size=size, batch=1)


@functools.lru_cache(maxsize=None)
def _fresh(size):
    """The prediction of a fresh two-scale flow model with refinement at ``size``."""
    return flags_gpu.run_gpu(_flow_s2rr(size))[0][0]


@pytest.mark.parametrize('sizes', [((96, 160), (160, 96), (96, 160)), ((160, 224), (64, 32), (160, 224))])
def test_geometry_changes_on_one_model(sizes):
    """One model runs three sizes in turn (96x160 and 160x96 have equal token counts at every scale; 160x224 and 64x32 are the
    largest and the smallest map of the matrix): every prediction has the bits of a fresh model's at that size.  A position table,
    workspace or plane cache keyed by token count and not by (h, w) fails here."""
    model = ff.build_model(_flow_s2rr(sizes[0])).to(DEV).set_precision('exact')
    for step, size in enumerate(sizes):
        case = _flow_s2rr(size)
        i0, i1, _ = ff.inputs(case)
        pred = model(i0.to(DEV), i1.to(DEV), **case.fwd)['flow_preds'][0].cpu()
        model.check_operand_range()
        want = _fresh(size)
        assert torch.equal(pred, want), (step, size, (pred - want).abs().max().item())


def test_sequence_at_an_odd_window_size():
    """``forward_sequence`` on three 80x112 frames (5x7 windows, one scale, both directions) agrees with the pairwise forwards: the
    comparison of test_sequence_against_pairwise at its own size."""
    from tests.test_video_gpu import floor_close
    from unimatch_amd.synth import synth_frames
    case = fs.BY_NAME['flow_s1_80x112']
    model = ff.build_model(case).to(DEV).set_precision('exact')
    kw = {k: v for k, v in case.fwd.items() if k != 'task'}
    frames = synth_frames(3, *case.size, seed=77).to(DEV)
    pairwise = [model(frames[i:i + 1], frames[i + 1:i + 2], pred_bidir_flow=True, **kw)['flow_preds'][0] for i in range(2)]
    out = model.forward_sequence(frames, pred_bidir_flow=True, **kw)
    model.check_operand_range()
    assert torch.isfinite(out['flow']).all() and tuple(out['flow'].shape) == (2, 2) + case.size
    for i in range(2):
        assert floor_close(out['flow'][i], pairwise[i][0]), i
        assert floor_close(out['flow_bwd'][i], pairwise[i][1]), i
