"""The as-rounded bf16 emulation (tests/bf16_emulation.py) checked alone, on the host: for every input set of
tests/test_fast_mode_parity_gpu.py, at the same shapes and seeds,

  1. with rounding switched off and in fp64 the emulation equals the oracle (oracle/hotpath.py) or the fp64 expression of the matching
     exact-mode test to 1e-12 of the output scale;
  2. mean|E32 - E64| (as-rounded emulation in fp32 against fp64) is at most 1/16 of the rounding noise it emulates, mean|E64 - T|, T the
     fp64 evaluation on rounded operands without intermediate rounding -- for every output whose kernel rounds something behind its
     operands.  gsv3 / gsv4, the LayerNorm and the fp32 epilogues round nothing there: for them E64 == T is asserted instead;
  3. the unmodified E32 passes the GPU file's gate and a copy with an injected defect fails it.

Multi-stage cases take the E64 planes of one stage as the next stage's operands, in the role the device's planes have on the GPU.
"""
import pytest
import torch

from tests import bf16_emulation as em
from tests import test_fast_mode_parity_gpu as gp

F64, F32 = torch.float64, torch.float32


def _self_check(case, tag):
    want = case.oracle()
    plain, _, _ = case.emulate(F64, False)
    assert set(plain) == set(want)
    for name in want:
        assert em.exact_close(plain[name], want[name]), (tag, name, (plain[name].double() - want[name]).abs().max().item())
    e64, bounds, planes = case.emulate(F64, True, want_bound=True)
    e32, _, _ = case.emulate(F32, True, planes=planes)
    t64, _, _ = case.emulate(F64, 'operands', planes=planes)
    for name in sorted(e64):
        st = em.gate(e32[name], e64[name], e32[name], bounds.get(name), case.floor(name, e64[name]), (tag, name))     # E32 passes
        noise = (e64[name] - t64[name]).abs()
        print(f'SELF {tag} | {name} | E32-E64 mean {st["ref_mean"]:.3e} max {st["ref_max"]:.3e} | '
              f'E64-T mean {noise.mean().item():.3e} max {noise.max().item():.3e}')
        if name in case.rounds:
            assert st['ref_mean'] <= noise.mean().item() / 16.0, (tag, name, st['ref_mean'], noise.mean().item())
        else:
            assert torch.equal(e64[name], t64[name]), (tag, name)
    return e64, e32, bounds


def _must_fail(case, name, bad, e64, e32, bounds, tag):
    with pytest.raises(AssertionError):
        em.gate(bad, e64[name], e32[name], bounds.get(name), case.floor(name, e64[name]), tag)


@pytest.mark.parametrize('kind,case', gp.WATTN_CASES)
def test_window_attention_emulation(kind, case):
    c = gp.WindowAttn(kind, case)
    e64, e32, bounds = _self_check(c, f'wattn-{kind}-{case}')
    n = c.geom[2] * c.geom[3]
    # defects: the last key of the (ragged) last key tile dropped; one 32-key tile counted twice (where the window has one to spare)
    mult = torch.ones(n)
    mult[n - 1] = 0.0
    defects = [mult] if n > 1 else []
    if n > 32:
        mult = torch.ones(n)
        mult[:32] = 2.0
        defects.append(mult)
    for mult in defects:
        bad, _, _ = c.emulate(F32, True, key_mult=mult)
        _must_fail(c, 'out', bad['out'], e64, e32, bounds, 'defect')


@pytest.mark.parametrize('kind,case', gp.ATTN_LAYER_CASES)
def test_attention_layer_emulation(kind, case):
    _self_check(gp.AttnLayer(kind, case), f'layer-{kind}-{case}')


@pytest.mark.parametrize('kind,case', gp.MATCHING_CASES)
def test_global_matching_emulation(kind, case):
    c = gp.Matching(kind, case)
    e64, e32, bounds = _self_check(c, f'match-{kind}-{case}')
    # defect: one split's partial rows left out of the combine -- the second half of the keys is missing
    L = c.h * c.w
    if L >= 2:
        mult = torch.ones(L, L)
        mult[:, L // 2:] = 0.0
        bad, _, _ = c.emulate(F32, True, key_mult=mult)
        for name in ('flow', 'prop2', 'prop1'):       # prop1: the (2 + 1)-float partial row
            _must_fail(c, name, bad[name], e64, e32, bounds, 'defect')


@pytest.mark.parametrize('mk', [(300, 128, 128), (257, 384, 128), (128, 1024, 256)])
def test_linear_planes_emulation(mk):
    _self_check(gp.LinearPlanes(mk), f'linear-planes-{mk}')


def test_linear_layernorm_emulation():
    _self_check(gp.LinearLn(), 'linear-ln')


@pytest.mark.parametrize('m,hidden', [(128, 1024), (333, 1024), (1000, 64), (4096 + 17, 512)])
def test_ffn_emulation(m, hidden):
    c = gp.Ffn(m, hidden)
    e64, e32, bounds = _self_check(c, f'ffn-{m}x{hidden}')
    mult = torch.ones(hidden)
    mult[hidden - 32:] = 0.0                          # defect: one 32-wide hidden chunk skipped
    bad, _, _ = c.emulate(F32, True, hidden_mult=mult)
    _must_fail(c, 'out', bad['out'], e64, e32, bounds, 'defect')


def test_ffn_kv_emulation():
    _self_check(gp.Ffn(1000, 1024, seed=1400), 'ffn-kv')


@pytest.mark.parametrize('m', [128, 1000, 2 * 6144 + 40])
def test_kv4_emulation(m):
    _self_check(gp.Kv4(m), f'kv4-{m}')


@pytest.mark.parametrize('m', [300, 257])
def test_linear_bias_emulation(m):
    _self_check(gp.LinearBias(m), f'linear-bias-{m}')


@pytest.mark.parametrize('shape', gp.PROJ_SHAPES)
def test_prop_projected_emulation(shape):
    c = gp.PropProjected(shape)
    _self_check(c, f'prop-projected-{shape}')
    lg = c.logits()
    assert 25.0 < lg.abs().max().item() < 60.0, lg.abs().max().item()        # logits reach about +-40 (30 .. 48 over the five shapes)
