"""``um_depth_corr_softmax_multi`` on the device: several source views vote in one plane sweep.

The fusion rule (csrc/depth_multi.hip): ``l_j = (sum_s v_sj l_sj) / max(1, n_j)`` over the sources that see candidate j, then one softmax.
Gates are those of tests/test_depth_stats_gpu.py: float planes within ``2e-4 * scale`` of the float64 restatement on the same float32
values (``scale`` 1 for ``max_prob`` / ``peak_mass``, ``max(1, ln D)`` for ``entropy``, ``max(cand)`` for ``out``, the candidate range squared
for ``variance``); ``best`` by value on every row and by equality where the float64 gap is at least 0.1; ``in_view`` on the pixels clear
of the crossing coordinates of every source (at least 90 % of them).  Bit-for-bit claims: S = 1 against the two-view kernels, a repeated
source and a masked source against S = 1.
"""
import math

import numpy as np
import pytest
import torch

from tests import depth_multiview_util as mv
from tests import memory_guard as mg
from unimatch_amd import _abi, confidence
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = mv.TOL


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


def multi(ops, f0, f1, h, w, cam, cand, use=None, from_argmax=False, **kw):
    """The backend's plane sweep on source-major operands ``[S, B, ...]``: one ``um_depth_corr_softmax_multi`` launch."""
    return ops.depth_corr_softmax(f0, f1, h, w, cam, cand, from_argmax, use=use, **kw)


def dev(*tensors):
    return tuple(t.to(DEV) for t in tensors)


compare = mv.compare              # the gates of the module docstring; rows 8 .. 11 of tests/test_dispatch_boundaries_gpu.py share them


# ------------------------------------------------------------------ 1. against float64
def test_the_inputs_have_the_properties_the_gates_need():
    mv.check_input_properties()


@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('case', list(mv.CASES))
def test_against_float64(ops, case, argmax):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    ref = mv.reference(case)
    got = multi(ops, *dev(f0, f1), h, w, *dev(cam, cand), None, argmax, stats=True)
    assert tuple(got[0].shape) == (b, 1, h, w) and tuple(got[1].shape) == (b, 4, h, w) and tuple(got[2].shape) == (b, 2, h, w)
    if argmax:
        assert torch.equal(got[0][:, 0], cand.to(DEV)[got[2][:, 0].long()])        # the read-out is the candidate at best
        ref = dict(ref, out=got[0].cpu().double())                                 # ... and `best` is gated below
    compare(got, ref, d, f'case {case} argmax={argmax}')


# ------------------------------------------------------------------ 2. S = 1 is the two-view kernels, bit for bit
@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('move', ['sideways', 'diagonal', 'forward'])
@pytest.mark.parametrize('d', [5, 64, 65, 128])
@pytest.mark.parametrize('b,h,w', [(2, 9, 11), (2, 16, 24)])
def test_one_source_is_the_two_view_kernel(ops, b, h, w, d, move, argmax):
    f0, f1 = dev(*mv.features(b, h, w, (move,)))
    cam, cand = dev(mv.cameras(b, h, w, (move,)), mv.candidates(d))
    want = ops.depth_corr_softmax(f0[0], f1[0], h, w, cam[0], cand, argmax, stats=True, peak_radius=2)
    got = multi(ops, f0, f1, h, w, cam, cand, None, argmax, stats=True, peak_radius=2)
    for name, a, e in zip(('out', 'stats', 'index'), got, want):
        assert torch.equal(a, e), (name, (a.double() - e.double()).abs().max().item())
    assert torch.equal(multi(ops, f0, f1, h, w, cam, cand, None, argmax), want[0])       # without the statistics


# ------------------------------------------------------------------ 3. repeated and permuted sources
@pytest.mark.parametrize('d,move', [(64, 'sideways'), (64, 'diagonal'), (17, 'forward'), (80, 'diagonal'), (128, 'sideways')])
def test_a_repeated_source_changes_nothing(ops, d, move):
    b, h, w = 2, 16, 24
    f0, f1 = dev(*mv.features(b, h, w, (move,)))
    cam, cand = dev(mv.cameras(b, h, w, (move,)), mv.candidates(d))
    one = multi(ops, f0, f1, h, w, cam, cand, stats=True)
    for times in (2, 4):
        many = multi(ops, f0.repeat(times, 1, 1, 1), f1.repeat(times, 1, 1, 1), h, w, cam.repeat(times, 1, 1), cand, stats=True)
        for a, e in zip(many, one):
            assert torch.equal(a, e), (times, (a.double() - e.double()).abs().max().item())


def test_the_order_of_the_sources_does_not_matter(ops):
    (b, h, w), d, moves = mv.CASES['B']
    f0, f1, cam, cand = dev(*mv.inputs('B'))
    want = multi(ops, f0, f1, h, w, cam, cand)
    for perm in ([1, 2, 0], [2, 1, 0]):
        got = multi(ops, f0[perm].contiguous(), f1[perm].contiguous(), h, w, cam[perm].contiguous(), cand)
        assert (got - want).abs().max().item() <= TOL * mv.scales(d)['out']


# ------------------------------------------------------------------ 4. use
@pytest.mark.parametrize('case', ['A', 'C'])
def test_a_source_that_is_off_is_never_read(ops, case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = dev(*mv.inputs(case))
    f0, f1, cam = f0[:2].clone(), f1[:2].clone(), cam[:2].clone()
    want = multi(ops, f0[:1].contiguous(), f1[:1].contiguous(), h, w, cam[:1].contiguous(), cand, stats=True)
    f0[1], f1[1], cam[1] = float('nan'), float('nan'), float('nan')
    use = torch.tensor([[1, 1], [0, 0]], dtype=torch.uint8, device=DEV)
    got = multi(ops, f0, f1, h, w, cam, cand, use, stats=True)
    for a, e in zip(got, want):
        assert torch.equal(a, e)


@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_a_mask_per_sample_against_float64(ops, case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    use = torch.ones(len(moves), b, dtype=torch.uint8)
    use[1, 1] = 0                                                                  # use[1] = [1, 0]
    ref = mv.reference_of(f0, f1, h, w, cam, cand, use)
    whole = mv.reference(case)
    assert (ref['out'][0] - whole['out'][0]).abs().max().item() <= 1e-12 and (ref['out'][1] - whole['out'][1]).abs().max().item() > 2e-3
    got = multi(ops, *dev(f0, f1), h, w, *dev(cam, cand, use), stats=True)
    compare(got, ref, d, f'case {case} use[1] = [1, 0]')


# ------------------------------------------------------------------ 5. nothing in view
@pytest.mark.parametrize('sources', [1, 2])
@pytest.mark.parametrize('d', [1, 17, 64, 65, 128])
@pytest.mark.parametrize('b,h,w', [(1, 1, 1), (2, 9, 11)])
def test_nothing_in_view_is_exactly_uniform(ops, b, h, w, d, sources):
    moves = ('away',) * sources
    f0, f1 = dev(*mv.features(b, h, w, moves))
    out, stats, index = (t.cpu() for t in multi(ops, f0, f1, h, w, *dev(mv.cameras(b, h, w, moves), mv.candidates(d)),
                                                                       stats=True))
    assert bool((index == 0).all())                                                # best == 0 and in_view == 0
    one_over = np.float32(1.0) / np.float32(d)
    assert (stats[:, 0].double() - 1.0 / d).abs().max().item() <= float(np.spacing(one_over))
    ln = np.float32(math.log(d))
    assert (stats[:, 1].double() - math.log(d)).abs().max().item() <= float(np.spacing(ln)) if d > 1 else bool((stats[:, 1] == 0).all())
    assert (out.double() - mv.candidates(d).double().mean()).abs().max().item() <= TOL * mv.scales(d)['out']


def test_a_sample_with_every_source_off_is_uniform(ops):
    (b, h, w), d, moves = mv.CASES['A']
    f0, f1, cam, cand = dev(*mv.inputs('A'))
    use = torch.tensor([[1, 0], [1, 0]], dtype=torch.uint8, device=DEV)
    out, stats, index = multi(ops, f0, f1, h, w, cam, cand, use, stats=True)
    assert bool((index[1] == 0).all()) and bool((index[0, 1] > 0).any())
    assert (stats[1, 0].double() - 1.0 / d).abs().max().item() <= float(np.spacing(np.float32(1.0) / np.float32(d)))


# ------------------------------------------------------------------ 6. optional outputs, 8. refusals (the C ABI)
def _abi_call(lib, f0, f1, cam, use, cand, out, stats, index, sources, b, h, w, c, d, argmax, radius):
    ptr = lambda t: None if t is None else t.data_ptr()
    return lib.um_depth_corr_softmax_multi(ptr(f0), ptr(f1), ptr(cam), ptr(use), ptr(cand), ptr(out), ptr(stats), ptr(index), sources, b,
                                           h, w, c, d, argmax, radius, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('case', ['B', 'C'])
def test_stats_and_index_are_optional_in_the_abi(case):
    (b, h, w), d, moves = mv.CASES[case]
    lib = _abi.load()
    f0, f1, cam, cand = dev(*mv.inputs(case))

    def call(with_stats, with_index):
        out = torch.full((b, 1, h, w), float('nan'), device=DEV)
        stats = torch.full((b, 4, h, w), -7.0, device=DEV)
        index = torch.full((b, 2, h, w), -7, dtype=torch.int32, device=DEV)
        _abi.check(_abi_call(lib, f0, f1, cam, None, cand, out, stats if with_stats else None, index if with_index else None, len(moves),
                             b, h, w, mv.C, d, 0, 1), 'um_depth_corr_softmax_multi')
        return out, stats, index

    out, stats, index = call(True, True)
    o1, s1, i1 = call(False, True)
    o2, s2, i2 = call(True, False)
    o3, s3, i3 = call(False, False)
    assert torch.equal(o1, out) and torch.equal(o2, out) and torch.equal(o3, out)
    assert torch.equal(i1, index) and torch.equal(s2, stats)
    assert bool((s1 == -7).all()) and bool((i2 == -7).all()) and bool((s3 == -7).all()) and bool((i3 == -7).all())     # not written


def test_refusals_launch_nothing():
    (b, h, w), d, moves = mv.CASES['A']
    lib = _abi.load()
    f0, f1, cam, cand = dev(*mv.inputs('A'))
    out = torch.full((b, 1, h, w), -7.0, device=DEV)
    good = dict(f0=f0, f1=f1, cam=cam, use=None, cand=cand, out=out, stats=None, index=None, sources=2, b=b, h=h, w=w, c=mv.C, d=d,
                argmax=0, radius=1)
    bad = [dict(sources=0), dict(sources=9), dict(d=0), dict(d=129), dict(radius=-1), dict(c=64), dict(f0=None), dict(f1=None),
           dict(cam=None), dict(cand=None), dict(out=None), dict(b=0)]
    for change in bad:
        assert _abi_call(lib, **dict(good, **change)) < 0, change
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                                 # nothing was launched
    assert _abi_call(lib, **good) == 0
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ 7. memory contract
def test_memory_contract():
    """Red zones intact, inputs unchanged, results identical across the fills: every byte of out, stats and index is written, nothing
    outside them, nothing read beyond the inputs.  Case B (box and gather sources in one pixel), case C (the gather kernel) and a
    source switched off for one sample."""

    def run(ops, g):
        res = []
        for case, masked, argmax in (('B', False, False), ('C', False, True), ('B', True, False), ('C', True, False)):
            (b, h, w), d, moves = mv.CASES[case]
            f0, f1, cam, cand = (g.place(t) for t in mv.inputs(case))
            use = None
            if masked:
                use = torch.ones(len(moves), b, dtype=torch.uint8)
                use[1, 0] = 0
                use = g.place(use)
            res += list(multi(ops, f0, f1, h, w, cam, cand, use, argmax, stats=True, peak_radius=2))
        return res

    first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps('exact'))
    assert first is not None
    assert any('ops.py' in site for site in mg.contract.last_sites)


# ------------------------------------------------------------------ the public function
def test_depth_match_multi_runs_the_kernel_on_cuda_tensors(ops):
    (b, h, w), d, moves = mv.CASES['A']
    f0, f1, cam, cand = dev(*mv.inputs('A'))
    from unimatch_amd.ops import KernelTimer
    ops.timer = timer = KernelTimer()
    out, st = confidence.depth_match_multi(f0, f1, h, w, cam, cand, ops=ops)
    ops.timer = None
    assert [r[0] for r in timer.records] == ['depth_corr_softmax_multi']
    want = multi(ops, f0, f1, h, w, cam, cand, stats=True)
    assert torch.equal(out, want[0]) and torch.equal(st.max_prob, want[1][:, 0]) and torch.equal(st.in_view, want[2][:, 1])


# ------------------------------------------------------------------ 9. the model
def _model(name):
    from unimatch_amd import UniMatch
    from unimatch_amd.synth import CONFIGS, synth_state_dict
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model = model.to(DEV).set_precision('exact')
    model.launch_parts = 1
    kw = dict(fk)
    kw.pop('task')
    return model, kw


def _depth_inputs(count, h, w, seed):
    from unimatch_amd.synth import synth_camera, synth_frames
    x = synth_frames(count, h, w, seed=seed) / 255.
    x = (x - torch.tensor((0.485, 0.456, 0.406)).view(1, 3, 1, 1)) / torch.tensor((0.229, 0.224, 0.225)).view(1, 3, 1, 1)
    k, rel = synth_camera(count - 1, h, w)
    return x.contiguous().to(DEV), k.to(DEV), rel.to(DEV)


@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_forward_multiview(name):
    from unimatch_amd.ops import KernelTimer
    model, kw = _model(name)
    x, k, rel = _depth_inputs(5, 64, 96, 2500)
    ref, nxt, prv = x[1:4].contiguous(), x[2:5].contiguous(), x[0:3].contiguous()
    pose_next, pose_prev = rel[1:4].contiguous(), torch.inverse(rel[0:3]).contiguous()
    plain = model(ref, nxt, task='depth', intrinsics=k[1:4], pose=pose_next, **kw)['flow_preds'][0]
    one = model.forward_multiview(ref, nxt[:, None], intrinsics=k[1:4], poses=pose_next[:, None], **kw)['flow_preds'][0]
    assert torch.equal(one, plain), (one - plain).abs().max().item()                       # S = 1 is forward, bit for bit
    srcs, poses = torch.stack([nxt, prv], 1).contiguous(), torch.stack([pose_next, pose_prev], 1).contiguous()
    model.debug_taps = taps = {}
    model.ops.timer = timer = KernelTimer()
    two = model.forward_multiview(ref, srcs, intrinsics=k[1:4], poses=poses, return_confidence=True, peak_radius=2, **kw)
    model.ops.timer = None
    model.debug_taps = None
    names = [r[0] for r in timer.records]
    assert names.count('depth_corr_softmax_multi') == 1 and 'depth_corr_softmax' not in names and 'depth_corr_softmax_stats' not in names
    depth = two['flow_preds'][0]
    assert tuple(depth.shape) == (3, 64, 96) and bool(torch.isfinite(depth).all())
    lo, hi = sorted((1. / kw.get('min_depth', 1. / 0.5), 1. / kw.get('max_depth', 1. / 10)))
    assert depth.min().item() >= lo * (1 - 1e-6) and depth.max().item() <= hi * (1 + 1e-6)
    floor = 1e-3 * max(1.0, plain.abs().max().item())
    assert (depth - plain).abs().amax((1, 2)).max().item() > floor                           # the second view has a say on some frame
    again = model.forward_multiview(ref, srcs, intrinsics=k[1:4], poses=poses, **kw)['flow_preds'][0]
    assert torch.equal(again, depth)                                                         # with and without the statistics, repeated
    # the confidence is that of the fused distribution of the tapped tokens
    h, w, d = 8, 12, 64
    tok0, tok1 = (taps[n].flatten(2).transpose(1, 2).contiguous() for n in ('f0_s0', 'f1_s0'))
    assert tok0.shape[0] == 6                                                                # B S pairs in one stream, source-major
    cam = model.ops.depth_cam(k[1:4].repeat(2, 1, 1), poses.transpose(0, 1).reshape(6, 4, 4).contiguous(), 8.0)
    cand = torch.linspace(kw.get('min_depth', 1. / 0.5), kw.get('max_depth', 1. / 10), d)
    f0, f1, cams = tok0.view(2, 3, h * w, 128), tok1.view(2, 3, h * w, 128), cam.view(2, 3, 30)
    ref64 = mv.reference_of(f0.cpu(), f1.cpu(), h, w, cams.cpu(), cand, peak_radius=2)
    conf = two['depth_confidence']
    assert conf['scale'] == 8 and conf['num_candidates'] == d
    stats = torch.stack([conf[key] for key in mv.FLOATS], 1)
    index = torch.stack([conf['best'], conf['in_view']], 1)
    out, _ = confidence.depth_match_multi(f0, f1, h, w, cams, cand.to(DEV), peak_radius=2, ops=model.ops)
    sc = dict(mv.scales(d), out=cand.max().item(), variance=(cand.max() - cand.min()).item() ** 2)
    got = (out.cpu(), stats.cpu(), index.cpu())
    dist = {'out': (got[0].double() - ref64['out']).abs().max().item()}
    for i, key in enumerate(mv.FLOATS):
        dist[key] = (got[1][:, i].double() - getattr(ref64['stats'], key)).abs().max().item()
    print(name, dist)
    for key, v in dist.items():
        assert v <= TOL * sc[key], (key, v)
    wide = ref64['gap'] >= 0.1
    assert torch.equal(got[2][:, 0].long()[wide], ref64['prob'].argmax(1)[wide])
    assert torch.equal(got[2][:, 1][ref64['clear']], ref64['stats'].in_view[ref64['clear']])
    # refusals
    with pytest.raises(ValueError, match='pred_bidir_depth'):
        model.forward_multiview(ref, srcs, intrinsics=k[1:4], poses=poses, pred_bidir_depth=True, **kw)
    with pytest.raises(ValueError, match="task='depth'"):
        model.forward_multiview(ref, srcs, intrinsics=k[1:4], poses=poses, task='flow', **kw)


def test_forward_multiview_never_synchronises():
    model, kw = _model('gmdepth_s1')
    x, k, rel = _depth_inputs(3, 64, 96, 2501)
    srcs = torch.stack([x[2:3], x[0:1]], 1).contiguous()
    poses = torch.stack([rel[1:2], torch.inverse(rel[0:1])], 1).contiguous()
    args = dict(intrinsics=k[1:2].contiguous(), poses=poses, return_confidence=True, **kw)
    model.forward_multiview(x[1:2], srcs, **args)                                            # warm: weight planes, position tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = model.forward_multiview(x[1:2], srcs, **args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert bool(torch.isfinite(out['flow_preds'][0]).all())
