"""k_proj / v_proj folded into the query and merge weights (``HipOps.fold_kv``) on the GPU.

* ``um_ffn_planes_fwd``: the FFN that also writes the operand planes of its result.  fp32 output BITWISE ``um_ffn_ws_fwd``'s, planes BITWISE
  the format pass (``split_planes_kernel``) of that output, in both operand precisions, on the tile kernel (``ffn_kernel<.., PLANES>``)
  and on the hidden-split fallback (split FFN + format pass inside the call); under red zones (tests/memory_guard.py).
* the whole ``FeatureTransformer``, folded and unfolded, against ``oracle.hotpath.feature_transformer`` in fp64 under the project's
  stage gate (tests/test_stage_parity_gpu.py: GPU error <= 2 x the fp32 port's + 4 fp32 ulps of the stage's magnitude, every sample),
  with the launches each forward made.

Identity and cache bookkeeping: tests/test_fold_kv_cpu.py.
"""
import ctypes

import pytest
import torch

from oracle import hotpath as hp
from tests import memory_guard as mg
from unimatch_amd import _abi
from unimatch_amd.model import FeatureTransformer, _to_map, _to_tokens
from unimatch_amd.ops import HipOps, KernelTimer
from unimatch_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ULP_FLOOR = 4 * 2.0 ** -24                     # tools/stage_parity.py: 4 fp32 ulps of the stage's mean magnitude
UM_K_SPLIT_PLANES, UM_K_LINEAR, UM_K_FFN = 2, 7, 10
# a launch is hidden-split while tiles x 2 fit the chip (ffn.hip: ffn_hidden_split), i.e. up to 128 tiles on 256 CUs; hidden = 64 has too
# few slices to split, so the small m reach the tile kernel there; at hidden = 1024 (the model's) m = 129 * 128 + 40 does, with a ragged tile
MS = (1, 127, 129, 1000)
BIG_M = 129 * 128 + 40


def _rnd(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _ffn_weights(hidden, place=lambda t: t):
    norm = torch.nn.LayerNorm(128)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(128, generator=torch.Generator().manual_seed(41)))
        norm.bias.copy_(0.1 * torch.randn(128, generator=torch.Generator().manual_seed(42)))
    norm = norm.to(DEV)
    return place(_rnd(43, hidden, 256, scale=0.06)), place(_rnd(44, 128, hidden, scale=0.03)), norm


@pytest.fixture(scope='module', params=['exact', 'fast'])
def ops(request):
    return HipOps(request.param)


@pytest.mark.parametrize('m,hidden', [(m, hid) for hid in (64, 1024) for m in MS] + [(BIG_M, 1024)])
def test_ffn_planes_is_the_ffn_plus_the_format_pass_bit_for_bit(ops, m, hidden):
    w1, w2, norm = _ffn_weights(hidden)
    x, y = _rnd(100 + m, m, 128, scale=1.5), _rnd(200 + m, m, 128, scale=1.5)
    want = ops.ffn_ln(x, y, w1, w2, norm)
    want_planes, rows, cols = ops.linear_planes(want, ())
    assert (rows, cols) == (m, 128) and want_planes.numel() == m * 128 * 2 * ops.nplanes
    lib = ops.lib
    lib.um_census_enable(1)
    try:
        got, planes = ops.ffn_ln(x, y, w1, w2, norm, planes=True)
        torch.cuda.synchronize()
        census = _abi.census(lib)
    finally:
        lib.um_census_enable(0)
    split = lib.um_ffn_split_workspace_bytes(m, hidden) > 0
    assert (census['ffn_hsplit'], census['ffn_tile']) == ((1, 0) if split else (0, 1)), (m, hidden, census)
    assert split == (hidden == 1024 and m != BIG_M), 'the cases are meant to reach both paths'
    assert torch.equal(got, want)
    assert torch.equal(planes, want_planes)
    if ops.precision == 'exact':                                   # what the planes mean: hi + lo is the fp32 value to 2^-22
        hi, lo = planes.view(torch.float16).view(2, m, 128).float()
        assert ((hi + lo) - want).abs().max() <= want.abs().max() * 2.0 ** -21
    _abi.check_operand_range()


@pytest.mark.parametrize('mode', ['exact', 'fast'])
def test_ffn_planes_under_red_zones(mode):
    """W / I / U / R and run-to-run equality of the raw bytes (tests/memory_guard.py) of ``ffn_ln(planes=True)`` and of the identity
    ``linear_planes`` on the tile kernel (hidden 64), the hidden-split fallback (hidden 1024) and ragged tiles: the planes buffer holds
    exactly ``m * 128 * 2 * NS`` bytes, so a row past ``m`` or a lo plane at a wrong stride lands in a red zone."""
    def run(ops, g):
        out = []
        for hidden in (64, 1024):
            w1, w2, norm = _ffn_weights(hidden, g.place)
            norm = g.place_module(norm)
            for m in (1, 127, 129, 257):
                x, y = g.place(_rnd(300 + m, m, 128, scale=1.5)), g.place(_rnd(400 + m, m, 128, scale=1.5))
                o, p = ops.ffn_ln(x, y, w1, w2, norm, planes=True)
                out += [o, p, ops.linear_planes(x, ())[0]]
        return out

    first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps(mode))
    assert first is not None
    assert any('ops.py' in s for s in mg.contract.last_sites)      # the product's allocations went through the guard


# ------------------------------------------------------------------------------------------------ whole FeatureTransformer
def _launch_counts(lib):
    out = {}
    for name, k in (('split_planes', UM_K_SPLIT_PLANES), ('linear', UM_K_LINEAR), ('ffn', UM_K_FFN)):
        ms, n = ctypes.c_double(), ctypes.c_int()
        assert lib.um_timing_collect(k, ctypes.byref(ms), ctypes.byref(n)) == 0
        out[name] = n.value
    return out


def _forward(net, ops, f0, f1, attn_type, splits):
    """The second forward on ``ops`` (the first builds the cached weight planes, which are format-pass launches too) -> (maps on the
    CPU, launches by HipOps wrapper, launches by kernel id inside the library)."""
    h, w = f0.shape[-2:]
    lib = ops.lib
    if not ops._wcache:
        net(ops, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, splits)
    ops.timer = KernelTimer()
    lib.um_timing_enable(-1)
    try:
        t0, t1 = net(ops, _to_tokens(f0.to(DEV)), _to_tokens(f1.to(DEV)), h, w, attn_type, splits)
        torch.cuda.synchronize()
        kernels = _launch_counts(lib)
    finally:
        lib.um_timing_enable(0)
    wrappers = {k: v['calls'] for k, v in ops.timer.summary().items()}
    ops.timer = None
    return (_to_map(t0, h, w).cpu(), _to_map(t1, h, w).cpu()), wrappers, kernels


@pytest.fixture(scope='module')
def transformer():
    net = FeatureTransformer()
    sd = synth_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=7)
    net.load_state_dict(sd)
    return net.to(DEV), sd


@pytest.mark.parametrize('h,w', [(24, 40), (32, 48)])
def test_folded_transformer_within_the_stage_gate(transformer, h, w):
    """2 pairs of h x w maps, swin K = 2 (ragged 32-key tiles, shifted classes that straddle tiles, table and probe paths).  Per output
    and per sample: mean |GPU - fp64| <= 2 x mean |fp32 port - fp64| + 4 fp32 ulps of mean |fp64| -- for the folded forward (the
    default) AND for the forward with the knob off (k | v projected: um_kv4_fwd / um_ffn_kv_fwd), in one test.

    Launches.  Knob on: no wrapper launch named 'linear' (the k | v projection is gone: one 'linear' launch less per forward, the format
    pass of block 0 in its place) and no linear-family kernel at all inside the library; the FFN launches of blocks 0..4 write the next
    block's planes (or run the format pass inside the call while the launch is hidden-split).  Knob off: as before this change."""
    net, sd = transformer
    g = torch.Generator().manual_seed(1000 + h)
    f0, f1 = torch.randn(2, 128, h, w, generator=g), torch.randn(2, 128, h, w, generator=g)
    sd64 = {k: v.double() for k, v in sd.items()}
    truth = hp.feature_transformer(f0.double(), f1.double(), sd64, 'swin', 2)
    port = hp.feature_transformer(f0, f1, sd, 'swin', 2)

    on = HipOps('exact')
    assert on.fold_kv
    off = HipOps('exact')
    off.fold_kv, off.fused_kv = False, True                        # the forward before the fold
    m = 4 * h * w
    inner = 5 if on.lib.um_ffn_split_workspace_bytes(m, 1024) > 0 else 0      # second launches inside the FFN calls of blocks 0..4
    results = {}
    for tag, ops_ in (('folded', on), ('unfolded', off)):
        maps, wrappers, kernels = _forward(net, ops_, f0, f1, 'swin', 2)
        results[tag] = maps
        print(f'{h}x{w} {tag}: wrappers {wrappers} kernels {kernels}')
        assert wrappers['window_attn'] == 12 and wrappers['ffn'] == 6 and kernels['ffn'] == 6, (tag, wrappers, kernels)
        if tag == 'folded':
            assert 'linear' not in wrappers and wrappers['split_planes'] == 1, wrappers
            assert kernels['linear'] == 0 and kernels['split_planes'] == 1 + inner, kernels
        else:
            assert wrappers['linear'] == 1 and 'split_planes' not in wrappers, wrappers
            assert kernels['linear'] == 1 + inner and kernels['split_planes'] == 0, kernels
        _abi.check_operand_range()
    assert sum(v for v in _forward(net, on, f0, f1, 'swin', 2)[1].values()) == 19

    bad = []
    for tag, maps in results.items():
        for which, got, want, p32 in zip(('f0', 'f1'), maps, truth, port):
            for n in range(want.shape[0]):
                e_gpu = (got[n].double() - want[n]).abs().mean().item()
                e_port = (p32[n].double() - want[n]).abs().mean().item()
                mag = want[n].abs().mean().item()
                line = f'{h}x{w} {tag:8s} {which}[{n}] |x| {mag:.3e} GPU {e_gpu:.3e} port {e_port:.3e} ratio {e_gpu / e_port:.2f}'
                print(line)
                if not e_gpu <= 2.0 * e_port + ULP_FLOOR * mag:
                    bad.append(line)
    assert not bad, '\n' + '\n'.join(bad)


def test_folded_transformer_1d_cross_attention_and_fast_mode(transformer):
    """The stereo model's layers (2-D swin self attention, whole-scanline 1-D cross attention with kv_rotate) folded, against fp64 under
    the same gate; and the folded forward in bf16 held to the unfolded forward in bf16 the way the gate holds the GPU to the port: its
    error against fp64 at most twice the unfolded one's.  (Both round every operand to bf16, 2^-9; the folded one rounds no projected
    key / value, so it has no reason to be further away.  A wiring error is O(1).)"""
    net, sd = transformer
    h, w = 24, 40
    g = torch.Generator().manual_seed(77)
    f0, f1 = torch.randn(1, 128, h, w, generator=g), torch.randn(1, 128, h, w, generator=g)
    truth = hp.feature_transformer(f0.double(), f1.double(), {k: v.double() for k, v in sd.items()}, 'self_swin2d_cross_1d', 2)
    port = hp.feature_transformer(f0, f1, sd, 'self_swin2d_cross_1d', 2)
    maps, _, kernels = _forward(net, HipOps('exact'), f0, f1, 'self_swin2d_cross_1d', 2)
    assert kernels['linear'] == 0
    for got, want, p32 in zip(maps, truth, port):
        e_gpu, e_port = (got.double() - want).abs().mean().item(), (p32.double() - want).abs().mean().item()
        print(f'1-D cross: GPU {e_gpu:.3e} port {e_port:.3e}')
        assert e_gpu <= 2.0 * e_port + ULP_FLOOR * want.abs().mean().item()
    fast_on, fast_off = HipOps('fast'), HipOps('fast')
    fast_off.fold_kv, fast_off.fused_kv = False, True
    a, _, _ = _forward(net, fast_on, f0, f1, 'swin', 2)
    b, _, _ = _forward(net, fast_off, f0, f1, 'swin', 2)
    want = hp.feature_transformer(f0.double(), f1.double(), {k: v.double() for k, v in sd.items()}, 'swin', 2)
    for x, y, t in zip(a, b, want):
        e_on, e_off = (x.double() - t).abs().mean().item(), (y.double() - t).abs().mean().item()
        print(f'fast: folded {e_on:.3e} unfolded {e_off:.3e} vs fp64')
        assert e_on <= 2.0 * e_off + ULP_FLOOR * t.abs().mean().item()
