"""The forward-size matrix (tests/forward_sizes.py) without a GPU: the reference's answers pin the oracle, the oracle pins the
product's host path, the fp32 oracle stays close enough to fp64 for the GPU gates to mean something -- and the matrix is shown to be
ABLE to fail: the host mirrors say which kernels and window geometries its rows reach (and that the three sizes every other
whole-model test runs reach none of them), and seeded defects of ``attention_windows`` that no older row notices break the gate here.
What remains unknown after this file is only the GPU leg (tests/test_forward_sizes_gpu.py).

Measured when the matrix was written: fp32 oracle vs the reference at most 7e-6 mean, product with OracleOps vs the fp32 oracle at most
2e-6 mean, fp32 vs fp64 oracle at most 4.4e-5 in any pixel (``E32_LIMIT`` is 1e-3)."""
import pytest
import torch

from tests import degenerate_content as dc
from tests import dispatch_boundaries as db
from tests import forward_flags as ff
from tests import forward_sizes as fs
from tests.oracle_ops import OracleOps
from tests.test_forward_flags_cpu import _distinguishing_calls


@pytest.mark.parametrize('name', fs.RUNNING)
def test_oracle_matches_the_reference(golden, name):
    """The gate of the flag matrix's test_oracle_matches_the_reference, unchanged, on the reference's fp32 prediction of the row."""
    case = fs.BY_NAME[name]
    g = golden(case.fixture)
    ref, spread = g[f'{name}.fp32'], float(g[f'{name}.spread'])
    out = fs.oracle(case, torch.float32)
    assert out.shape == ref.shape
    err = (out - ref).abs().mean().item()
    assert err < max(5 * spread, 1e-5), (name, err, spread)


def test_the_fixtures_hold_the_rows_and_nothing_else(golden):
    assert fs.RAISING == [] and len(fs.RUNNING) == len(fs.CASES)          # every row runs in the reference, so HipOps must serve it
    for fixture in fs.FIXTURES:
        want = {f'{c.name}.{part}' for c in fs.CASES if c.fixture == fixture for part in ('fp32', 'spread')}
        assert set(golden(fixture).keys()) == want, fixture


def _host_path_error(case):
    """The product's host path with the CPU oracle as backend against ``unimatch_forward`` in fp32 -> (mean abs error, the backend)."""
    i0, i1, cam = ff.inputs(case)
    ops = OracleOps()
    model = ff.build_model(case).bind_ops(ops)
    pred = model(i0, i1, **case.fwd, **cam)['flow_preds'][0]
    want = fs.oracle(case, torch.float32) if case.name in fs.BY_NAME else ff.oracle(case, torch.float32)
    assert pred.shape == want.shape
    return (pred - want).abs().mean().item(), ops


@pytest.mark.parametrize('name', fs.RUNNING)
def test_product_host_path_matches_the_oracle(name):
    """The gate and the distinguishing calls of the flag matrix's test of the same name, unchanged: mean abs < 1e-5."""
    case = fs.BY_NAME[name]
    err, ops = _host_path_error(case)
    assert err < 1e-5, (name, err)
    called = {c[0] for c in ops.calls}
    must, never = _distinguishing_calls(case)
    assert must <= called and not (never & called), (name, sorted(called))
    if case.ctor['reg_refine']:
        assert sum(c[0] == 'local_corr_with_flow' for c in ops.calls) == case.fwd['num_reg_refine']


@pytest.mark.parametrize('name', fs.RUNNING)
def test_rows_are_conditioned(name):
    """``max|fp32 oracle - fp64 oracle| <= E32_LIMIT``: plain fp32 arithmetic answers the row, so the GPU gates (a few times the fp32
    oracle's error plus a floor) separate a defect from rounding."""
    case = fs.BY_NAME[name]
    d = (fs.oracle(case, torch.float32).double() - fs.oracle(case, torch.float64)).abs()
    assert d.max().item() <= dc.E32_LIMIT, (name, d.max().item())


# ------------------------------------------------------------------ what makes the matrix able to fail
def _windows_2d(size, num_scales, splits_list):
    return {g for g in fs.windows(size, num_scales, 'swin', splits_list)}


def _windows_1d(size, num_scales, splits_list):
    return {g for g in fs.windows(size, num_scales, 'self_swin2d_cross_swin1d', splits_list)} - _windows_2d(size, num_scales, splits_list)


def _reach(rows):
    """``rows``: (size, num_scales, splits_list, reg_refine) -> what the host rules take over all of them."""
    r = dict(kinds={64: set(), 96: set(), 128: set()}, rows_parts=[], win2d=set(), win1d=set(), maps=set(), l8=set(), k4m=set(), gru=set())
    for size, ns, splits, refine in rows:
        for cout, kind in fs.encoder_kinds(size, ns).items():
            r['kinds'][cout].add(kind)
        r['rows_parts'] += [(size,) + p for p in fs.rows_parts_feed_a_norm(size, ns)]
        r['win2d'] |= {g for g in _windows_2d(size, ns, splits) if (g[2], g[3]) != (g[0], g[1])}       # (full attention has no window)
        r['win1d'] |= _windows_1d(size, ns, splits)
        r['maps'] |= set(fs.maps(size, ns))
        r['l8'].add(size[0] // 8 * (size[1] // 8))
        if refine:
            r['k4m'].add(fs.refine_on_whole_tiles(size, ns))
            r['gru'].add(fs.gru_kind(size, ns))
    return r


def test_what_the_matrix_reaches():
    """Computed from the host mirrors (``db.conv_kind``, ``db.conv_parts``, ``attention_windows``), over the matrix as a whole."""
    m = _reach((c.size, c.ctor['num_scales'], c.fwd['attn_splits_list'], c.ctor['reg_refine']) for c in fs.CASES)
    # every convolution kernel at each of the encoder's three widths
    assert all(kinds == {'patch', 'rows', 'generic'} for kinds in m['kinds'].values()), m['kinds']
    # the row-window kernel's statistics parts feed a norm, and their count is not what the patch kernel would have left
    assert m['rows_parts'] and any(parts != patch_parts for _, _, parts, patch_parts in m['rows_parts']), m['rows_parts']
    win = m['win2d']
    assert any(g[2] % 2 for g in win) and any(g[3] % 2 for g in win), sorted(win)                    # odd window height, odd width
    assert any(g[4] % 2 for g in win) and any(g[5] % 2 for g in win)                                 # an odd shift in each axis
    assert any(2 * g[4] != g[2] and g[4] for g in win) and any(2 * g[5] != g[3] and g[5] for g in win)   # ... and a rounded one
    assert any((g[4] == 0) != (g[5] == 0) for g in win)                                              # a shift of zero in one axis only
    assert any(g[2] * g[3] > 128 for g in win) and any(g[2] * g[3] < 32 for g in win)                # two query tiles | below a key tile
    assert any(g[3] % 2 for g in m['win1d']) and all(g[2] == 1 for g in m['win1d'])                  # 1-D windows of odd length
    assert any(h > w for h, w in m['maps'])                                                          # portrait
    assert any(l % 64 == 0 for l in m['l8']) and any(l % 64 for l in m['l8']) and any(l % 32 for l in m['l8']), sorted(m['l8'])
    assert m['k4m'] == {True, False}                                                                 # refinement maps on whole tiles | not
    assert m['gru'] == {'rows', 'generic'}                                                           # GRU gates from 256 pixels on | below


def test_the_old_sizes_reach_none_of_it():
    """The three geometries of every other whole-model test (64x96 one scale, 128x192 two scales, 96x128 depth; with one and two
    splits and the refinement on): no row-window convolution in the encoder, so none of its statistics parts in front of a norm; the
    generic kernel only for the 128-channel layer; every window with even sides, hence no rounded shift (their one odd shift, 3,
    is half of 6); no shift that is zero in one axis only."""
    splits = {1: ([2], [1]), 2: ([2, 8],)}
    old = _reach((size, ns, sp, True) for size, ns in fs.OLD_SIZES for sp in splits[ns])
    assert not any('rows' in kinds for kinds in old['kinds'].values()), old['kinds']
    assert old['kinds'][64] == {'patch'} and old['kinds'][96] == {'patch'} and old['kinds'][128] <= {'patch', 'generic'}
    assert old['rows_parts'] == []
    win = old['win2d'] | old['win1d']
    assert win and not any(g[2] % 2 or g[3] % 2 for g in old['win2d']) and not any(g[3] % 2 for g in old['win1d']), sorted(win)
    assert not any((g[4] and 2 * g[4] != g[2]) or (g[5] and 2 * g[5] != g[3]) for g in win)
    assert not any((g[4] == 0) != (g[5] == 0) for g in old['win2d'])


# ------------------------------------------------------------------ seeded defects of attention_windows
def _mutant(which, real):
    """``attention_windows`` with one defect that only an odd or a portrait window sees."""
    def mutated(attn_type, is_self, splits, h, w, with_shift):
        wh, ww, sh, sw = real(attn_type, is_self, splits, h, w, with_shift)
        two_d = attn_type == 'swin' or (attn_type in ('self_swin2d_cross_1d', 'self_swin2d_cross_swin1d') and is_self)
        one_d = attn_type == 'self_swin2d_cross_swin1d' and not is_self
        if not with_shift or splits <= 1:
            return wh, ww, sh, sw
        if which == 'ceil_shift_2d' and two_d:
            return wh, ww, (wh + 1) // 2, (ww + 1) // 2
        if which == 'ceil_shift_1d' and one_d:
            return wh, ww, sh, (ww + 1) // 2
        if which == 'portrait_shift_swapped' and two_d and wh > ww:
            return wh, ww, ww // 2, wh // 2
        return wh, ww, sh, sw
    return mutated


# the defect -> a row of this matrix that must notice it (an odd 2-D window; a 1-D window of 7 tokens; a 12x4 window)
MUTANTS = {'ceil_shift_2d': 'flow_s1_80x112', 'ceil_shift_1d': 'stereo_s1_80x112', 'portrait_shift_swapped': 'flow_s2_bidir_192x64'}


@pytest.mark.parametrize('which', sorted(MUTANTS))
def test_seeded_defects_pass_the_flag_matrix_and_fail_here(monkeypatch, which):
    """A shift rounded up instead of down (2-D windows; 1-D cross-attention windows) and a shift whose axes are swapped in portrait
    windows, seeded into the product's ``attention_windows`` and run through OracleOps: every row of the flag matrix stays within its
    1e-5 gate (its windows have even sides and lie landscape), the named row of this matrix breaks that gate.  Measured: 0.67 at
    flow_s1_80x112 for the 2-D ceil shift."""
    from unimatch_amd import model as um_model
    monkeypatch.setattr(um_model, 'attention_windows', _mutant(which, um_model.attention_windows))
    for name in ff.RUNNING:
        err, _ = _host_path_error(ff.BY_NAME[name])
        assert err < 1e-5, (which, name, err)
    err, _ = _host_path_error(fs.BY_NAME[MUTANTS[which]])
    print(f'SIZES | mutant | {which} | {MUTANTS[which]} | mean abs error {err:.3e}')
    assert err >= 1e-5, (which, MUTANTS[which], err)
