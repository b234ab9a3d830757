"""Degenerate content (tests/degenerate_content.py) without a GPU: the builders give what they promise, the oracle's answers on ties
have the closed form a uniform softmax must give, the forwards stay well conditioned (so the absolute gates of the GPU leg mean
something), and the product's host path passes those gates with the oracle as backend."""
import pytest
import torch

from oracle import hotpath as hp
from tests import degenerate_content as dc
from tests import forward_flags as ff
from tests.oracle_ops import OracleOps
from tests.test_forward_flags_gpu import ARGMAX_TOL, check_gates

F = torch.nn.functional


# ------------------------------------------------------------------ the builders
@pytest.mark.parametrize('name', ['flow_s1_split1', 'stereo_s1_swin', 'flow_s2_rr2_b2'])
def test_pairs_hold_what_the_table_says(name):
    case = ff.BY_NAME[name]
    t0, t1, _ = ff.inputs(case)
    flow = ff.task_of(case) == 'flow'
    value = lambda v: dc.pixel(case, v).expand_as(t0)
    h, w = case.size
    for kind in dc.KINDS:
        i0, i1 = dc.pair(case, kind)
        assert i0.shape == t0.shape and i1.shape == t1.shape and i0.dtype == torch.float32 and i0.is_contiguous() and i1.is_contiguous()
        assert torch.isfinite(i0).all() and torch.isfinite(i1).all()
    if flow:
        assert dc.pixel(case, 128).flatten().tolist() == [128.0] * 3
    else:
        assert (dc.pixel(case, 255).flatten() - torch.tensor([(1 - m) / s for m, s in zip(dc.IMAGENET_MEAN, dc.IMAGENET_STD)])).abs().max() < 1e-6
    for kind, v0, v1 in (('black', 0, 0), ('white', 255, 255), ('grey_vs_black', 128, 0)):
        i0, i1 = dc.pair(case, kind)
        assert torch.equal(i0, value(v0)) and torch.equal(i1, value(v1)), kind
    i0, i1 = dc.pair(case, 'identical')
    assert torch.equal(i0, t0) and torch.equal(i1, i0) and i1.data_ptr() != i0.data_ptr()
    i0, i1 = dc.pair(case, 'fade')
    assert torch.equal(i0, t0) and torch.equal(i1, value(0))
    for img, tex in zip(dc.pair(case, 'letterbox'), (t0, t1)):
        assert torch.equal(img[..., :h // 4, :], value(0)[..., :h // 4, :]) and torch.equal(img[..., h - h // 4:, :], value(0)[..., :h // 4, :])
        assert torch.equal(img[..., h // 4:h - h // 4, :], tex[..., h // 4:h - h // 4, :])
    for img, tex in zip(dc.pair(case, 'half_flat'), (t0, t1)):
        assert torch.equal(img[..., :w // 2], value(128)[..., :w // 2]) and torch.equal(img[..., w // 2:], tex[..., w // 2:])
    i0, i1 = dc.pair(case, 'sensor_noise')
    assert not torch.equal(i0, i1)
    if flow:
        assert set(i0.unique().tolist()) == {0.0, 1.0, 2.0} and set(i1.unique().tolist()) == {0.0, 1.0, 2.0}
    else:
        assert i0[:, 0].unique().numel() == 3
    if case.batch > 1:
        assert not torch.equal(i0[0], i0[1])


def test_matrix_is_the_one_the_gpu_leg_runs():
    assert len(dc.MATRIX) == 6 * 8 + 2 * 4 + 1 == len(set(dc.MATRIX))
    assert all(n in ff.RUNNING and k in dc.KINDS for n, k in dc.MATRIX) and dc.TWO_PARTS in dc.MATRIX


def test_frames_repeat_cut_and_letterbox():
    f = dc.frames('mixed')
    h, w = dc.SEQUENCE_SIZE
    assert tuple(f.shape) == (5, 3, h, w) and f.is_contiguous()
    assert torch.equal(f[0], f[1]) and not f[2].any() and not torch.equal(f[3], f[0])
    assert not f[4, :, :h // 4].any() and not f[4, :, h - h // 4:].any() and torch.equal(f[4, :, h // 4:h - h // 4], f[3, :, h // 4:h - h // 4])


def test_channel_patterns_hold_what_the_table_says():
    b, c, h, w = 2, 64, 37, 29
    x = dc.channel_patterns(b, c, h, w, seed=1)
    assert tuple(x.shape) == (b, c, h, w) and x.dtype == torch.float32 and torch.isfinite(x).all()
    assert torch.equal(x, dc.channel_patterns(b, c, h, w, seed=1)) and not torch.equal(x, dc.channel_patterns(b, c, h, w, seed=2))
    n = h * w
    flat = x.view(b, c, n)
    assert [flat[0, ch, 0].item() for ch in (0, 8, 16, 24)] == [2.5, 0.0, -1000.0, 2.5]
    for ch in range(0, c, 8):
        assert flat[:, ch].unique().numel() == 1                                   # P0
        one = flat[:, ch + 1]                                                       # P1
        assert int((one == 2.75).sum()) == b and int((one == 2.5).sum()) == b * (n - 1)
        assert int(torch.nonzero(one[0] == 2.75)) == (0, n - 1, n // 2)[(ch // 8) % 3]
        two = x[:, ch + 2]                                                          # P2: every row is constant, two levels
        assert (two == two[..., :1]).all() and two.unique().numel() == 2
        assert torch.equal(two[:, 0], two[:, -1]) and not torch.equal(two[:, 0], two[:, h // 2])
    std = x.double().flatten(2).std(-1)
    mean = x.double().flatten(2).mean(-1)
    pat = dc.pattern_of(c)
    ratio = (mean / std).abs()
    assert 80 < ratio[:, pat == 3].min() and ratio[:, pat == 3].max() < 125
    assert 800 < ratio[:, pat == 4].min() and ratio[:, pat == 4].max() < 1250
    assert bool((x[:, pat == 5][:, :, 0, 0] == 1000.0).all()) and x[:, pat == 5].flatten(2)[..., 1:].abs().max() < 6
    assert x.double()[:, pat == 6].flatten(2).var(-1).max() < 2e-3 * 1e-5                     # 1e-8: far below eps
    assert (std[:, pat == 7] - 1).abs().max() < 0.1
    for p in range(3, 8):                                                           # samples differ: a swap cannot hide
        assert not torch.equal(x[0, pat == p], x[1, pat == p])
    # fp64 says 0 on the constant channels (torch's fp64 mean of 1073 times -1000 is off by an ulp: 1e-13 x rstd)
    assert F.instance_norm(x.double())[:, pat == 0].abs().max() < 1e-9
    small = dc.channel_patterns(1, 8, 12, 16, seed=3)
    assert dc.pattern_of(8).tolist() == list(range(8)) and small[0, 0].unique().tolist() == [2.5]


@pytest.mark.parametrize('cout,hw,stride', [(64, (15, 21), 1), (96, (7, 9), 1), (64, (22, 60), 1), (64, (47, 63), 2), (64, (16, 64), 1)])
def test_pattern_weights_carry_the_patterns_through_a_convolution(cout, hw, stride):
    """The weights the convolution-fed statistics tests use put the patterns into the convolution's output (fp64): constant P0 planes,
    border included, P1's single pixel, P6's variance, mean / sigma above 50 and 500 -- and the outputs beyond the inputs are zero-mean
    mixtures.  Plain ``0.01 * randn`` cross-talk does not: no plane stays constant."""
    x = dc.channel_patterns(3, 64, *hw, seed=4300).double()
    wt, bias = dc.pattern_conv_weights(cout, 64, 3, 4301)
    assert bool((wt[torch.arange(64), torch.arange(64), 1, 1] > 0.9).all()) and (wt != 0).float().mean() > 0.05
    y = F.conv2d(x, wt.double(), bias.double(), stride=stride, padding=1)
    dc.check_output_patterns(y, 64)
    if cout > 64:
        mix = y[:, 64:].flatten(2)
        assert (mix.mean(-1) / mix.std(-1)).abs().max() < 30
    plain = 0.01 * torch.randn(cout, 64, 3, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    plain[torch.arange(64), torch.arange(64), 1, 1] += 1.0
    with pytest.raises(AssertionError, match='P0 is not constant'):
        dc.check_output_patterns(F.conv2d(x, plain, None, stride=stride, padding=1), 64)


def test_token_rows_and_maps():
    x, group = dc.token_rows(333, 128, seed=5)
    assert set(group.tolist()) == {0, 1, 2, 3}
    assert not x[group == 0].any() and x[group == 3].abs().min() > 0
    ident = torch.nonzero(group == 1).flatten()
    assert torch.equal(x[ident], x[ident[:1]].expand(len(ident), 128))
    assert any(len(set(group[i:i + 32].tolist())) > 1 for i in range(0, 320, 32))
    for kind in dc.TOKEN_KINDS:
        f0, f1 = dc.token_maps(kind, 2, 7, 9)
        assert tuple(f0.shape) == tuple(f1.shape) == (2, 128, 7, 9) and f0.is_contiguous() and f1.is_contiguous()
    f0, f1 = dc.token_maps('identical', 2, 7, 9)
    assert torch.equal(f0, f1) and bool((f0 == f0[:, :, :1, :1]).all()) and not torch.equal(f0[0], f0[1])
    f0, _ = dc.token_maps('two_level', 1, 7, 9)
    assert bool((f0[..., :4] == f0[..., :1]).all()) and bool((f0[..., 4:] == f0[..., 4:5]).all()) and not torch.equal(f0[..., 0], f0[..., 8])
    _, f1 = dc.token_maps('duplicated', 2, 7, 9)
    t1 = f1.flatten(2).transpose(1, 2)
    partner = dc.duplicate_partner(63)
    assert torch.equal(t1[:, partner], t1) and partner[32:].tolist() == list(range(31)) and partner[:32].tolist() == list(range(32))
    assert t1[0].unique(dim=0).shape[0] == 32


# ------------------------------------------------------------------ the closed form of a uniform softmax, in fp64
@pytest.mark.parametrize('kind', ['identical', 'zero'])
def test_uniform_softmax_gives_the_centroid_of_the_allowed_keys(kind):
    """Equal logits: the expected coordinate is the centroid of the keys that take part -- all keys (global flow, propagation), the keys
    x' <= x of the scanline (stereo), the in-image taps (local correlation), the window (attention)."""
    b, h, w = 2, 7, 9
    f0, f1 = (t.double() for t in dc.token_maps(kind, b, h, w))
    grid = hp.pixel_grid(h, w, torch.float64)
    flow = hp.global_corr_softmax_flow(f0, f1, True)
    want = dc.uniform_centroid(h, w).view(1, 2, 1, 1) - grid[None]
    assert (flow - want).abs().max().item() < 1e-12
    disp = hp.global_corr_softmax_stereo(f0, f1)
    assert (disp - (grid[0] / 2)[None, None]).abs().max().item() < 1e-12                 # x - mean(0 .. x) = x / 2
    r = 4
    local = hp.local_corr_softmax(f0, f1, r)
    xs, ys = grid[0], grid[1]
    # the in-image taps of pixel x run from max(-r, -x) to min(r, w - 1 - x): their mean offset
    cx = (torch.clamp(xs + r, max=w - 1) + torch.clamp(xs - r, min=0)) / 2 - xs
    cy = (torch.clamp(ys + r, max=h - 1) + torch.clamp(ys - r, min=0)) / 2 - ys
    assert (local - torch.stack([cx, cy], 0)[None]).abs().max().item() < 1e-12
    val = torch.randn(b, 2, h, w, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    prop = hp.prop_global(f1, val, {f'feature_flow_attn.{n}_proj.{p}': (torch.eye(128, dtype=torch.float64) if p == 'weight' else
                                                                        torch.zeros(128, dtype=torch.float64)) for n in 'qk' for p in ('weight', 'bias')})
    assert (prop - val.mean((2, 3), keepdim=True)).abs().max().item() < 1e-12
    # one unshifted window geometry: every token gets the mean value of its window
    s_, hh, ww, wh, wwin = 2, 12, 20, 6, 10
    q, k = (t.double().flatten(2).transpose(1, 2) for t in dc.token_maps(kind, s_, hh, ww))
    v = torch.randn(s_, hh * ww, 128, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    att = hp.window_attention(q, k, v, hh, ww, wh, wwin).view(s_, hh, ww, 128)
    vm = v.view(s_, hh // wh, wh, ww // wwin, wwin, 128).mean((2, 4), keepdim=True).expand(s_, hh // wh, wh, ww // wwin, wwin, 128)
    assert (att - vm.reshape(s_, hh, ww, 128)).abs().max().item() < 1e-12


# ------------------------------------------------------------------ whole forwards
@pytest.mark.parametrize('name,kind', dc.MATRIX, ids=[f'{n}-{k}' for n, k in dc.MATRIX])
def test_forwards_stay_well_conditioned(name, kind):
    """The fp32 oracle stays within 1e-3 of the fp64 oracle on every (case, kind): the condition that makes the GPU leg's absolute gates
    meaningful.  The margin is thin and the figure depends on the machine (the fp32 summation order): the largest per-sample maxima
    seen are 8.35e-4 (flow_s2_rr2_b2 on sensor noise, profiles/degenerate_content.txt), 7.2e-4 and 6.6e-4 (the same case on black
    frames, two other machines) -- 17 % below the limit at worst.  ``depth_s1_argmax``: no pixel beyond ``ARGMAX_TOL`` in fp32."""
    case = ff.BY_NAME[name]
    truth, f32 = dc.oracle(case, kind, torch.float64), dc.oracle(case, kind, torch.float32)
    assert torch.isfinite(truth).all() and torch.isfinite(f32).all()
    d = (f32.double() - truth).abs()
    print(f'{name} {kind}: e32 mean {d.mean().item():.2e} max {d.max().item():.2e}')
    assert d.max().item() <= dc.E32_LIMIT, (name, kind, d.max().item())
    if case.fwd.get('depth_from_argmax'):
        assert int((d > ARGMAX_TOL).sum()) == 0, (name, kind, d.max().item())


@pytest.mark.parametrize('name,kind', dc.MATRIX, ids=[f'{n}-{k}' for n, k in dc.MATRIX])
def test_product_host_path_passes_the_gates(name, kind):
    """The product's own forward on CPU tensors (the oracle as backend) under the gates of the GPU leg, against the same two answers."""
    case = ff.BY_NAME[name]
    i0, i1 = dc.pair(case, kind)
    model = ff.build_model(case).bind_ops(OracleOps())
    with torch.no_grad():
        pred = model(i0, i1, **case.fwd, **ff.inputs(case)[2])['flow_preds'][0]
    check_gates(case, pred, (dc.oracle(case, kind, torch.float64), dc.oracle(case, kind, torch.float32)), tag=' ' + kind)
