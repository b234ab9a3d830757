"""The forward-flag matrix: flag sets ``UniMatch.forward`` accepts beyond the canonical ones of ``synth.CONFIGS``, as plain data plus
the helpers that build a case's weights, inputs and oracle answers.  No pytest in here: ``tests/golden/make_golden_flags.py`` (the
reference's answers), ``tests/test_forward_flags_cpu.py`` and ``tests/test_forward_flags_gpu.py`` all read this one table.

Every case uses ``CONDITIONED`` weights (soft softmaxes: fp32 agrees with fp64 to ~1e-5, so absolute gates mean something), the
'shift' image pair, and a size the end-to-end GPU tests already run (64x96 one scale, 128x192 two scales, 96x128 depth).
"""
import functools
from collections import namedtuple

import torch

from oracle import model as om
from unimatch_amd import UniMatch
from unimatch_amd.synth import CONDITIONED, synth_camera, synth_images, synth_state_dict

Case = namedtuple('Case', 'name ctor fwd size batch seed fixture raises')

_S1 = dict(num_scales=1, upsample_factor=8, reg_refine=False)
_S1R = dict(num_scales=1, upsample_factor=8, reg_refine=True)
_S2 = dict(num_scales=2, upsample_factor=4, reg_refine=False)
_S2R = dict(num_scales=2, upsample_factor=4, reg_refine=True)
_TWO = dict(attn_splits_list=[2, 8], corr_radius_list=[-1, 4], prop_radius_list=[-1, 1])
_DEPTH = dict(attn_type='swin', task='depth', min_depth=0.1, max_depth=2.0, num_depth_candidates=16)


def _case(name, ctor, task, fwd, size, batch=1, seed=1000, fixture='flags', raises=None):
    return Case(name, dict(ctor, task=task), dict(fwd, task=task), size, batch, seed, fixture, raises)


def _one(splits, corr, prop):
    return dict(attn_splits_list=[splits], corr_radius_list=[corr], prop_radius_list=[prop])


# the reference's predictions are spread over three fixtures so that every committed file stays small
CASES = [
    _case('flow_s2', _S2, 'flow', dict(_TWO, attn_type='swin'), (128, 192)),
    _case('stereo_s2', _S2, 'stereo', dict(_TWO, attn_type='self_swin2d_cross_swin1d'), (128, 192)),
    _case('flow_s2_bidir', _S2, 'flow', dict(_TWO, attn_type='swin', pred_bidir_flow=True), (128, 192), fixture='flags_bidir'),
    _case('flow_s2_rr3_bidir', _S2R, 'flow', dict(_TWO, attn_type='swin', num_reg_refine=3, pred_bidir_flow=True), (128, 192),
          fixture='flags_bidir'),
    _case('flow_s2_rr2_b2', _S2R, 'flow', dict(_TWO, attn_type='swin', num_reg_refine=2), (128, 192), batch=2, fixture='flags_b2'),
    _case('stereo_s2_rr2_b2', _S2R, 'stereo', dict(_TWO, attn_type='self_swin2d_cross_swin1d', num_reg_refine=2), (128, 192), batch=2,
          fixture='flags_b2'),
    _case('flow_s1_split1', _S1, 'flow', dict(_one(1, -1, -1), attn_type='swin'), (64, 96)),
    _case('flow_s1_local', _S1, 'flow', dict(_one(2, 2, 1), attn_type='swin'), (64, 96)),
    _case('flow_s1_plain_attn', _S1, 'flow', dict(_one(2, -1, 2), attn_type='full'), (64, 96)),
    _case('stereo_s1_local', _S1, 'stereo', dict(_one(2, 4, 1), attn_type='self_swin2d_cross_1d'), (64, 96)),
    _case('stereo_s1_swin', _S1, 'stereo', dict(_one(2, -1, -1), attn_type='swin'), (64, 96)),
    _case('depth_s1_argmax', _S1, 'depth', dict(_DEPTH, attn_splits_list=[2], prop_radius_list=[-1], depth_from_argmax=True), (96, 128)),
    _case('depth_s1_localprop', _S1, 'depth', dict(_DEPTH, attn_splits_list=[1], prop_radius_list=[1]), (96, 128)),
    _case('depth_s1_rr2_bidir', _S1R, 'depth', dict(_DEPTH, attn_splits_list=[2], prop_radius_list=[-1], num_reg_refine=2,
                                                    pred_bidir_depth=True), (96, 128)),
    # the reference fails in a view (its features are not stacked at scale 0); the product refuses the flags
    _case('flow_s1_rr_bidir', _S1R, 'flow', dict(_one(2, -1, -1), attn_type='swin', pred_bidir_flow=True), (64, 96), raises='RuntimeError'),
]
BY_NAME = {c.name: c for c in CASES}
RUNNING = [c.name for c in CASES if c.raises is None]
RAISING = [c.name for c in CASES if c.raises is not None]
ORACLE_THREADS = 8


def task_of(case):
    return case.fwd['task']


@functools.lru_cache(maxsize=None)
def _state_dict(ctor_items):
    model = UniMatch(**dict(ctor_items))
    return synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED)


def state_dict(case):
    """The case's seeded weights (shared between cases of one constructor; treat as read-only)."""
    return _state_dict(tuple(sorted(case.ctor.items())))


def build_model(case):
    model = UniMatch(**case.ctor).eval()
    model.load_state_dict(state_dict(case))
    return model


def inputs(case):
    """``(img0, img1, camera)``: fp32 CPU tensors; ``camera`` is ``dict(intrinsics=, pose=)`` for depth, else empty."""
    h, w = case.size
    i0, i1 = synth_images(case.batch, h, w, seed=case.seed, kind='shift', normalized=task_of(case) != 'flow')
    cam = {}
    if task_of(case) == 'depth':
        k, pose = synth_camera(case.batch, h, w)
        cam = dict(intrinsics=k, pose=pose)
    return i0, i1, cam


def run_oracle(case, i0, i1, cam, dtype):
    """``oracle.model.unimatch_forward`` with the case's weights and flags on the given images (and camera) in ``dtype``, uncached."""
    kw = dict(case.fwd, num_scales=case.ctor['num_scales'], upsample_factor=case.ctor['upsample_factor'],
              reg_refine=case.ctor['reg_refine'], **{k: v.to(dtype) for k, v in cam.items()})
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, ORACLE_THREADS))
    try:
        with torch.no_grad():
            return om.unimatch_forward(state_dict(case), i0.to(dtype), i1.to(dtype), **kw)
    finally:
        torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype):
    case = BY_NAME[name]
    return run_oracle(case, *inputs(case), dtype)


def oracle(case, dtype=torch.float64):
    """``oracle.model.unimatch_forward`` of the case on the CPU in ``dtype``, computed once per process and shared: do not modify."""
    return _oracle(case.name, dtype)
