"""The forward-size matrix: ``UniMatch.forward`` at image sizes whose per-size host rules no other whole-model test reaches -- ragged
maps, windows with odd sides, windows of more than one query tile, portrait maps, maps below one tile -- as plain data plus the host
mirrors that say what each size takes.  No pytest in here: ``tests/golden/make_golden_sizes.py`` (the reference's answers),
``tests/test_forward_sizes_cpu.py``, ``tests/test_forward_sizes_gpu.py`` and ``tools/forward_sizes_table.py`` all read this one table.

Rows are ``forward_flags.Case`` records (``ff.state_dict``, ``ff.build_model``, ``ff.inputs`` and ``ff.run_oracle`` work unchanged):
``CONDITIONED`` weights, the 'shift' image pair, seed 1000.  The oracle answers are cached here (``oracle``), per process, because
``ff.oracle`` looks its cases up in the flag table.
"""
import functools

import torch

from tests import dispatch_boundaries as db
from tests import forward_flags as ff
from tests.forward_flags import _DEPTH, _S1, _S1R, _S2, _S2R, _TWO, _case, _one

_SWIN1D = 'self_swin2d_cross_swin1d'


def _depth(splits, prop, **more):
    return dict(_DEPTH, attn_splits_list=[splits], prop_radius_list=[prop], **more)


# the reference's predictions are spread over four fixtures so that every committed file stays small
CASES = [
    # 2x4 map, 1x2 windows with shift (0, 1), L = 8: the only row whose 64-channel layer is below the row-window kernel's 256 pixels
    _case('flow_s1_16x32', _S1, 'flow', dict(_one(2, -1, -1), attn_type='swin'), (16, 32), fixture='sizes_a'),
    _case('flow_s1_32x32', _S1, 'flow', dict(_one(2, -1, -1), attn_type='swin'), (32, 32), batch=3, fixture='sizes_a'),
    _case('flow_s1_48x80_local', _S1, 'flow', dict(_one(2, 2, 1), attn_type='swin'), (48, 80), fixture='sizes_a'),
    _case('depth_s1_48x80', _S1, 'depth', _depth(1, -1), (48, 80), fixture='sizes_a'),
    _case('flow_s1_80x112', _S1, 'flow', dict(_one(2, -1, -1), attn_type='swin'), (80, 112), fixture='sizes_a'),
    _case('stereo_s1_80x112', _S1, 'stereo', dict(_one(2, -1, -1), attn_type=_SWIN1D), (80, 112), fixture='sizes_a'),
    _case('stereo_s1rr_80x112', _S1R, 'stereo', dict(_one(2, -1, -1), attn_type='self_swin2d_cross_1d', num_reg_refine=2), (80, 112),
          fixture='sizes_a'),
    _case('depth_s1rr_112x176', _S1R, 'depth', _depth(2, -1, num_reg_refine=1), (112, 176), fixture='sizes_a'),
    _case('depth_s1_bidir_112x176', _S1R, 'depth', _depth(2, 1, num_reg_refine=1, pred_bidir_depth=True), (112, 176), batch=2,
          fixture='sizes_a'),
    _case('flow_s2rr_96x160_b2', _S2R, 'flow', dict(_TWO, attn_type='swin', num_reg_refine=2), (96, 160), batch=2, fixture='sizes_b'),
    _case('stereo_s2rr_160x96', _S2R, 'stereo', dict(_TWO, attn_type=_SWIN1D, num_reg_refine=2), (160, 96), fixture='sizes_b'),
    _case('flow_s2rr_160x224', _S2R, 'flow', dict(_TWO, attn_type='swin', num_reg_refine=2), (160, 224), fixture='sizes_b'),
    _case('flow_s2rr_64x32', _S2R, 'flow', dict(_TWO, attn_type='swin', num_reg_refine=2), (64, 32), fixture='sizes_b'),
    _case('flow_s2_bidir_64x64', _S2, 'flow', dict(_TWO, attn_type='swin', pred_bidir_flow=True), (64, 64), fixture='sizes_c'),
    _case('flow_s2_bidir_192x64', _S2, 'flow', dict(_TWO, attn_type='swin', pred_bidir_flow=True), (192, 64), fixture='sizes_c'),
    _case('stereo_s2rr_224x96', _S2R, 'stereo', dict(_TWO, attn_type=_SWIN1D, num_reg_refine=2), (224, 96), fixture='sizes_c'),
    _case('flow_s1rr_128x288', _S1R, 'flow', dict(_one(2, -1, -1), attn_type='swin', num_reg_refine=2), (128, 288), fixture='sizes_d'),
    _case('stereo_s1rr_128x288', _S1R, 'stereo', dict(_one(2, 4, 1), attn_type='self_swin2d_cross_1d', num_reg_refine=2), (128, 288),
          fixture='sizes_d'),
]
BY_NAME = {c.name: c for c in CASES}
RUNNING = [c.name for c in CASES if c.raises is None]
RAISING = [c.name for c in CASES if c.raises is not None]
FIXTURES = sorted({c.fixture for c in CASES})

# the three geometries every other whole-model test runs (model size, scales): what the coverage assertions compare with
OLD_SIZES = (((64, 96), 1), ((128, 192), 2), ((96, 128), 1))


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype):
    case = BY_NAME[name]
    return ff.run_oracle(case, *ff.inputs(case), dtype)


def oracle(case, dtype=torch.float64):
    """``oracle.model.unimatch_forward`` of the row on the CPU in ``dtype``, computed once per process and shared: do not modify."""
    return _oracle(case.name, dtype)


def answers(case):
    """The (fp64, fp32) oracle answers in the form ``check_gates`` / ``sample_errors`` of tests/test_forward_flags_gpu.py take."""
    return oracle(case, torch.float64), oracle(case, torch.float32)


# ------------------------------------------------------------------ what a size takes: host mirrors
def maps(size, num_scales):
    """The feature maps of the matching loop, low -> high resolution: ``[(h, w)]`` at 1/8 (and 1/4 with two scales)."""
    h, w = size
    return [(h // 8, w // 8)] if num_scales == 1 else [(h // 8, w // 8), (h // 4, w // 4)]


def windows(size, num_scales, attn_type, splits_list):
    """Every distinct attention geometry of the Transformer over all scales and both layer roles, shifted and not:
    ``{(map_h, map_w, win_h, win_w, shift_h, shift_w)}`` (``unimatch_amd.model.attention_windows``, as FeatureTransformer calls it)."""
    from unimatch_amd.model import attention_windows
    out = set()
    for (h, w), splits in zip(maps(size, num_scales), splits_list):
        for shift in (False, True) if ('swin' in attn_type and splits > 1) else (False,):
            for is_self in (True, False):
                out.add((h, w) + tuple(attention_windows(attn_type, is_self, splits, h, w, shift)))
    return out


def case_windows(case):
    return windows(case.size, case.ctor['num_scales'], case.fwd.get('attn_type', 'swin'), case.fwd['attn_splits_list'])


def encoder_convs(size, num_scales, entry=True, on_load=True):
    """Every ``um_conv2d*`` launch of ``CNNEncoder._forward_nhwc`` on an image of ``size``, in order, as ``[(layer, cout, (ho, wo),
    kind, normalises on load)]`` with ``kind`` from ``db.conv_kind``.  The 7x7 stem packs the image itself and then always launches
    the generic tiling (conv.hip's conv7_impl), whatever ``conv_kind`` would say of a 7x7 geometry.  A stride-2 block behind an identity-shortcut block runs its first convolution and projection as ONE launch of the generic tiling
    (``um_conv2d_entry_supported``: 96- and 128-wide tiles; ``HipOps.fused_entry``); a block's second convolution normalises on load
    where the patch kernel serves it at a tile of 64 columns or more (``um_conv2d_norm_supported``; ``HipOps.norm_on_load``)."""
    h, w = (size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1
    cin, identity, out = 64, False, [('conv1', 64, (h, w), 'generic', False)]
    blocks = (('layer1.0', 64, 1), ('layer1.1', 64, 1), ('layer2.0', 96, 2), ('layer2.1', 96, 1),
              ('layer3.0', 128, 2 if num_scales == 1 else 1), ('layer3.1', 128, 1))
    for name, cout, stride in blocks:
        proj = stride != 1 or cin != cout
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        k1, nt1 = db.conv_kind(h, w, cout, 3, 3, stride, 1, 1)
        fused = entry and proj and stride == 2 and identity and k1 == 'generic' and nt1 in (3, 4)
        out.append((name + ('.entry' if fused else '.conv1'), cout, (ho, wo), k1, False))
        k2, nt2 = db.conv_kind(ho, wo, cout, 3, 3, 1, 1, 1)
        out.append((name + '.conv2', cout, (ho, wo), k2, on_load and k2 == 'patch' and nt2 >= 2))
        if proj and not fused:
            out.append((name + '.proj', cout, (ho, wo), db.conv_kind(h, w, cout, 1, 1, stride, 0, 0)[0], False))
        h, w, cin, identity = ho, wo, cout, not proj
    out.append(('conv2', 128, (h, w), db.conv_kind(h, w, 128, 1, 1, 1, 0, 0)[0], False))
    for i in range(num_scales if num_scales > 1 else 0):
        s = 2 ** i
        out.append((f'trident/{s}', 128, ((h - 1) // s + 1, (w - 1) // s + 1), db.conv_kind(h, w, 128, 3, 3, s, 1, 1)[0], False))
    return out


def encoder_census(size, num_scales):
    """The launch census ``encoder_convs`` predicts: ``{conv_patch, conv_patch_norm, conv_rows, conv_generic: launches}`` (an
    on-load launch counts as a patch launch too, conv.hip's launch_conv_patch)."""
    convs = encoder_convs(size, num_scales)
    return {'conv_patch': sum(k == 'patch' for _, _, _, k, _ in convs), 'conv_patch_norm': sum(n for _, _, _, _, n in convs),
            'conv_rows': sum(k == 'rows' for _, _, _, k, _ in convs), 'conv_generic': sum(k == 'generic' for _, _, _, k, _ in convs)}


def encoder_kinds(size, num_scales):
    """The kernel of the stride-1 3x3 convolutions at each of the encoder's three widths: ``{64: kind, 96: kind, 128: kind}``
    (64 channels at 1/2, 96 at 1/4, 128 at 1/8 -- 1/4 with two scales): the second convolution of each layer's blocks."""
    return {cout: kind for name, cout, _, kind, _ in encoder_convs(size, num_scales) if name.endswith('.1.conv2')}


def rows_parts_feed_a_norm(size, num_scales):
    """The ``db.conv_parts`` of every row-window convolution of the encoder whose fused statistics feed ``um_nhwc_stats_finalize``
    (every block convolution: ``stats=True`` in encoder.py) -> ``[(layer, parts, parts the patch kernel would leave)]``."""
    return [(name, db.conv_parts(kind, ho, wo), db.conv_parts('patch', ho, wo))
            for name, _, (ho, wo), kind, _ in encoder_convs(size, num_scales) if kind == 'rows' and name.startswith('layer')]


def gru_kind(size, num_scales):
    """The kernel of the refinement block's 1x5 gate convolutions (256 outputs z | r, 128 outputs q: both 128-wide tiles) on the
    highest-resolution map: 'rows' from 256 pixels on, else 'generic' (conv.hip's conv_pick, rows5)."""
    h, w = maps(size, num_scales)[-1]
    kinds = {db.conv_kind(h, w, cout, 1, 5, 1, 0, 2)[0] for cout in (256, 128)}
    assert len(kinds) == 1
    return kinds.pop()


def attention_launches(case):
    """The Transformer's attention launches of one forward, ``[(streams, map_h, map_w, win_h, win_w)]``: six blocks of a self and a
    cross layer per scale, odd blocks shifted (FeatureTransformer.forward); the stream holds both images of every pair, and both
    directions from the second scale on with ``pred_bidir_flow`` (UniMatch._match)."""
    from unimatch_amd.model import attention_windows
    attn_type, out = case.fwd.get('attn_type', 'swin'), []
    for s, ((h, w), splits) in enumerate(zip(maps(case.size, case.ctor['num_scales']), case.fwd['attn_splits_list'])):
        streams = 2 * case.batch * (2 if case.fwd.get('pred_bidir_flow') and s > 0 else 1)
        for i in range(6):
            shift = 'swin' in attn_type and splits > 1 and i % 2 == 1
            for is_self in (True, False):
                out.append((streams, h, w) + tuple(attention_windows(attn_type, is_self, splits, h, w, shift))[:2])
    return out


def ffn_launches(case):
    """``[tokens]`` of the Transformer's FFN launches of one forward (one per block and scale, on the whole stream)."""
    return [s * h * w for s, h, w, _, _ in attention_launches(case)[1::2]]


def gsv_side(nbatch, tokens, causal, cus):
    """global_match.hip's launch_gsv restated: gsv4 where the launch is not causal, the keys are whole 64-key tiles (512 at least) and
    there are 8 units of (256 queries x 64 keys) per CU, else gsv3.  ``cus``: the device's CU count, read there and never written down."""
    units = nbatch * ((tokens + 255) // 256) * (tokens // 64)
    return 'gsv4' if (not causal and tokens % 64 == 0 and tokens >= 512 and units >= 8 * cus) else 'gsv3'


def matching_sides(case, cus, k4m_supported):
    """The census sides the layers after the Transformer must show: ``{'gsv3' | 'gsv4', 'k3_mfma' | 'k3_valu', 'k4_mfma' | 'k4_valu':
    launches or None for 'at least one'}``; a side that must NOT show maps to 0.  ``k4m_supported(h, w, channels, radius)``: the
    exported ``um_local_corr_with_flow_feat_supported``."""
    task, fwd, b = ff.task_of(case), case.fwd, case.batch
    bidir = bool(fwd.get('pred_bidir_flow') or fwd.get('pred_bidir_depth'))
    gsv, k3 = set(), {'k3_mfma': 0, 'k3_valu': 0}
    scale_maps = maps(case.size, case.ctor['num_scales'])
    for s, (h, w) in enumerate(scale_maps):
        radius = -2 if task == 'depth' else fwd['corr_radius_list'][s]
        if radius == -1 and task == 'stereo':
            gsv.add(gsv_side(b * h, w, True, cus))                          # one causal softmax per scanline
        elif radius == -1:
            sides = {gsv_side(n, h * w, False, cus) for n in (b, 2 * b)}    # (one or both directions in the launch)
            assert len(sides) == 1, (case.name, 'the side depends on how the directions are batched')
            gsv |= sides
        elif radius > 0:
            k3['k3_mfma' if task != 'stereo' and k4m_supported(h, w, 128, radius) else 'k3_valu'] += 1
        if fwd['prop_radius_list'][s] <= 0:
            gsv.add(gsv_side(2 * b if bidir else b, h * w, False, cus))
    out = dict(k3, gsv3=None if 'gsv3' in gsv else 0, gsv4=None if 'gsv4' in gsv else 0, k4_mfma=0, k4_valu=0)
    if case.ctor['reg_refine']:
        h, w = scale_maps[-1]
        out['k4_mfma' if k4m_supported(h, w, 128, 4) else 'k4_valu'] = fwd['num_reg_refine']
    return out


def refine_on_whole_tiles(size, num_scales):
    """``um_local_corr_with_flow_feat_supported`` at radius 4 restated (local_corr_mfma.hip:573: whole tiles of 4 rows x 8 columns):
    the matrix-core cost volume serves the refinement map, else the VALU kernel."""
    h, w = maps(size, num_scales)[-1]
    return h % 4 == 0 and w % 8 == 0
