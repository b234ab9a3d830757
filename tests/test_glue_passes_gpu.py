"""The copy / add / format passes between neighbouring kernels that ``HipOps.fused_glue`` removes.  None may change one bit:

* the stem fed two image tensors (``um_stem_conv_pair_fwd``) against the stem of their concatenation;
* the periodic addend of the convolution epilogue (``um_conv2d_addend_fwd``) against the plain launch plus the repeated table;
* the concatenation kernel (``um_nhwc_concat_planes``) against fill + permute + cat + format conversion, byte for byte;
* the upsampler head, and the whole model, with the knob on and off (one and two concurrent parts, both precisions; a two-scale
  refinement model, which takes none of the position shortcut; position-free taps);
* the launch table: two ``um_nhwc_instance_norm`` calls less per forward and no ``torch.cat`` of device tensors left in the encode
  step, the upsampler head and the join of the parts.
"""
import sys

import pytest
import torch

from unimatch_amd import UniMatch, _abi
from unimatch_amd.model import _to_map
from unimatch_amd.ops import HipOps
from unimatch_amd.synth import CONFIGS, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


def build(name, precision='exact'):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    return model.to(DEV).set_precision(precision), dict(fk)


# ------------------------------------------------------------------ the stem of two image tensors
@pytest.mark.parametrize('normalize', [False, True], ids=['raw', 'input_norm'])
@pytest.mark.parametrize('batches', [(1, 1), (2, 1)])
@pytest.mark.parametrize('hw', [(40, 56), (37, 51)])
def test_pair_stem_equals_the_stem_of_the_concatenation(ops, hw, batches, normalize):
    weight = rnd(11, 64, 3, 7, 7, scale=0.05).to(DEV)
    a = (rnd(12, batches[0], 3, *hw).abs() * 90.0).clamp(0, 255).to(DEV)
    b = (rnd(13, batches[1], 3, *hw).abs() * 90.0).clamp(0, 255).to(DEV)
    norm = NORM if normalize else None
    want, ho, wo = ops.stem_conv(torch.cat([a, b], 0), weight, norm, stats=True)
    want_stats, want_parts = ops.last_conv_stats
    got, ho2, wo2 = ops.stem_conv((a, b), weight, norm, stats=True)
    got_stats, got_parts = ops.last_conv_stats
    assert (ho, wo, want_parts) == (ho2, wo2, got_parts)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert torch.equal(got_stats, want_stats)


# ------------------------------------------------------------------ the periodic addend
# 12 x 20: P = 240, one full and one ragged 112-row tile per image; 8 x 16: P = 128 exactly; 64 channels: the other tile width
@pytest.mark.parametrize('channels,hw', [(128, (12, 20)), (128, (8, 16)), (64, (12, 20))])
def test_periodic_addend_equals_the_plain_launch_plus_the_table(ops, channels, hw):
    b, (h, w) = 3, hw
    x = rnd(21, b * h * w, channels, scale=1.5).to(DEV)
    weight = rnd(22, channels, channels, 1, 1, scale=0.1).to(DEV)
    bias = rnd(23, channels).to(DEV)
    pos = rnd(24, h * w, channels).to(DEV)
    planes, _ = ops.nhwc_norm(x, b, h * w, normalize=False, relu=False, want_planes=True)
    plain, _, _ = ops.conv2d_nhwc((planes, b, h, w, channels), weight, bias, 1, (0, 0))
    got, _, _ = ops.conv2d_nhwc((planes, b, h, w, channels), weight, bias, 1, (0, 0), image_addend=pos)
    assert torch.isfinite(got).all()
    assert torch.equal(got, plain + pos.repeat(b, 1))


# ------------------------------------------------------------------ the concatenation kernel
@pytest.mark.parametrize('v', [2, 1])
def test_concat_planes_are_bytewise_the_cat_and_apply_planes(ops, v):
    b, h, w, c = 2, 12, 20, 128
    rows = b * h * w
    flow = rnd(31, b, v, h, w, scale=20.0).to(DEV)
    feat = rnd(32, rows, c).to(DEV)
    want, want_c = ops.nhwc_planes_from([flow.permute(0, 2, 3, 1).reshape(rows, v), feat])
    got, got_c = ops.nhwc_concat_planes(flow, feat)
    assert got_c == want_c == 160 and got.numel() == want.numel() == 2 * (rows + 1) * 160 * 2
    assert torch.equal(got, want)                                  # pad columns and the zero row included


# ------------------------------------------------------------------ the upsampler head
def _head_inputs(b=2, h=12, w=20):
    tok0 = rnd(41, b, h * w, 128).to(DEV)
    flow = rnd(42, b, 2, h, w, scale=10.0).to(DEV)
    return flow, _to_map(tok0, h, w)


def test_upsampler_head_is_bitwise_the_same_with_the_knob_on_and_off(monkeypatch):
    model, _ = build('gmflow_s1')
    flow, f0_map = _head_inputs()
    out = {}
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(HipOps, 'fused_glue', on)
            mask, nhwc = model._upsample_mask(flow, f0_map)
            assert nhwc and tuple(mask.shape) == (2 * 12 * 20, 9 * 64)
            out[on] = (mask, model._upsample(flow, f0_map))
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])


def test_depth_upsampling_is_bitwise_the_same_with_the_knob_on_and_off(monkeypatch):
    model, _ = build('gmdepth_s1')
    flow, f0_map = _head_inputs()
    pad = torch.cat([flow[:, :1].abs() + 0.1, torch.zeros_like(flow[:, :1])], 1)
    out = {}
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(HipOps, 'fused_glue', on)
            out[on] = model._upsample(pad, f0_map, is_depth=True)
    assert torch.isfinite(out[True]).all() and torch.equal(out[True], out[False])


# ------------------------------------------------------------------ the model
def _forward_twice(model, i0, i1, kw):
    """Two forwards: with two parts the first one runs them one after the other, the second one on two streams."""
    with torch.no_grad():
        first = model(i0, i1, **kw)['flow_preds'][0]
        second = model(i0, i1, **kw)['flow_preds'][0]
    torch.cuda.synchronize()
    return first, second


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('parts', [1, 2])
def test_model_is_bitwise_the_same_with_the_knob_on_and_off(monkeypatch, parts, precision):
    i0, i1 = (t.to(DEV) for t in synth_images(2, 64, 96, seed=1000, kind='shift'))
    out = {}
    for on in (False, True):
        monkeypatch.setattr(HipOps, 'fused_glue', on)
        model, kw = build('gmflow_s1', precision)
        model.launch_parts = parts
        out[on] = _forward_twice(model, i0, i1, kw)
    for a, b in zip(out[True], out[False]):
        assert tuple(a.shape) == (2, 2, 64, 96) and torch.isfinite(a).all()
        assert torch.equal(a, b)
    assert torch.equal(out[True][0], out[True][1])


def test_two_scale_refinement_model_takes_no_position_shortcut(monkeypatch):
    i0, i1 = (t.to(DEV) for t in synth_images(2, 64, 96, seed=1000, kind='shift'))
    out, seen = {}, []
    for on in (False, True):
        monkeypatch.setattr(HipOps, 'fused_glue', on)
        model, kw = build('gmflow_s2_rr6')
        match = model._match
        monkeypatch.setattr(model, '_match', lambda *a, _m=match, **k: (seen.append((on, k.get('stream_has_pos'))), _m(*a, **k))[1])
        out[on] = _forward_twice(model, i0, i1, kw)
    assert seen and not any(has_pos for _, has_pos in seen)
    for a, b in zip(out[True], out[False]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_debug_taps_keep_position_free_backbone_features(monkeypatch):
    i0, i1 = (t.to(DEV) for t in synth_images(2, 64, 96, seed=1000, kind='shift'))
    taps = {}
    for on in (False, True):
        monkeypatch.setattr(HipOps, 'fused_glue', on)
        model, kw = build('gmflow_s1')
        model.debug_taps = {}
        with torch.no_grad():
            model(i0, i1, **kw)
        taps[on] = model.debug_taps
    assert torch.equal(taps[True]['backbone0_s0'], taps[False]['backbone0_s0'])
    assert torch.equal(taps[True]['backbone1_s0'], taps[False]['backbone1_s0'])
    # ... and they are the encoder's own output, without the table
    model, _ = build('gmflow_s1')
    with torch.no_grad():
        plain = model._encode((i0, i1))[0]
    assert torch.equal(taps[True]['backbone0_s0'], plain[:2]) and torch.equal(taps[True]['backbone1_s0'], plain[2:])


# ------------------------------------------------------------------ the launch table
ZONES = ('_encode', '_upsample_mask', 'run_parts', '_forward_one')


def _zone():
    """The innermost of ZONES on the Python stack: where a torch.cat call comes from."""
    f = sys._getframe(2)
    while f is not None:
        if f.f_code.co_name in ZONES:
            return f.f_code.co_name
        f = f.f_back
    return None


def test_launch_table_loses_two_format_passes_and_every_concatenation(monkeypatch):
    lib = _abi.load()
    i0, i1 = (t.to(DEV) for t in synth_images(2, 64, 96, seed=1000, kind='shift'))
    counts = {'norm': 0}
    cats = []
    norm, cat = lib.um_nhwc_instance_norm, torch.cat

    def w_norm(*a):
        counts['norm'] += 1
        return norm(*a)

    def w_cat(tensors, *a, **k):
        if any(t.is_cuda for t in tensors):
            cats.append(_zone())
        return cat(tensors, *a, **k)

    seen = {}
    for on in (False, True):
        monkeypatch.setattr(HipOps, 'fused_glue', on)
        model, kw = build('gmflow_s1')
        model.launch_parts = 2
        _forward_twice(model, i0, i1, kw)                          # the caches (weight planes, position table) exist from here on
        monkeypatch.setattr(lib, 'um_nhwc_instance_norm', w_norm)
        monkeypatch.setattr(torch, 'cat', w_cat)
        counts['norm'] = 0
        del cats[:]
        with torch.no_grad():
            model.launch_parts = 1
            model(i0, i1, **kw)
            one_forward = counts['norm']
            model.launch_parts = 2
            model(i0, i1, **kw)
        torch.cuda.synchronize()
        monkeypatch.setattr(lib, 'um_nhwc_instance_norm', norm)
        monkeypatch.setattr(torch, 'cat', cat)
        seen[on] = (one_forward, list(cats))
    assert seen[False][0] - seen[True][0] == 2, seen
    for zone in ('_encode', '_upsample_mask', 'run_parts'):
        assert zone in seen[False][1], (zone, seen[False][1])      # the counter sees the parent's concatenations
        assert zone not in seen[True][1], (zone, seen[True][1])
