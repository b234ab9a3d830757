"""GPU tests of the frame synthesis: ``um_image_warp``, ``um_flow_splat`` and ``um_frame_synthesize`` (csrc/interp.hip) are BITWISE
equal to the host restatement of ``unimatch_amd/interp.py`` -- integer accumulators, masks, averaged flows, uint8 frames, float32 warps.

Shapes (the smallest at which each mechanism can break):
  2x2 B=2      the entry points' minimum
  5x3 B=1      odd, smaller than a wave
  33x47 B=2    odd sizes, rows that are no multiple of 4, 1551 pixels: six full 256-thread blocks and a ragged seventh
  64x97 B=3    several images, 6208 pixels
with K = 1 (t = 0.5) and K = 3 (0.25, 0.5, 0.75), both image layouts.  Flows: a smooth pair with planted exact integer landings (taps of
weight zero), landings exactly on the last row and column, the bad inputs of tests/interp_util.py (NaN, +-inf, 1e9, 40000 px; weights
NaN / 0 / -1 / 7 / +-inf), and -- at 33x47 -- every pixel of both directions landing on ONE destination at t = 0.5 (maximum contention:
1551 adders per accumulator word).  The host results are computed once per case and shared."""
import ctypes

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, interp
from tests import interp_util as iu
from tests import memory_guard as mg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(2, 2, 2), (1, 5, 3), (2, 33, 47), (3, 64, 97)]
TIMES = {1: [0.5], 3: [0.25, 0.5, 0.75]}
CASES = [(b, h, w, k, 'mixed') for b, h, w in SHAPES for k in (1, 3)] + [(2, 33, 47, 1, 'converge'), (2, 33, 47, 3, 'converge')]
IDS = [f'{b}x{h}x{w}-K{k}-{kind}' for b, h, w, k, kind in CASES]


def make_flows(b, h, w, kind):
    """``(fwd, bwd, weight_fwd, weight_bwd)`` on the host."""
    seed = 100 * h + w
    fwd, bwd = iu.smooth_pair(b, h, w, seed)
    if kind == 'converge':                               # p + 0.5 flow(p) = the centre, for every pixel of both directions
        ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
        one = torch.stack([2.0 * (w // 2 - xs), 2.0 * (h // 2 - ys)], 0)
        fwd = one[None].repeat(b, 1, 1, 1).contiguous()
        return fwd, fwd.clone(), None, None
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
    fwd[:, 0, 0, :], fwd[:, 1, 0, :] = 4.0, 2.0          # row 0: integer landings at every t of the test (taps of weight zero)
    bwd[:, 0, 0, :], bwd[:, 1, 0, :] = -4.0, 0.0
    fwd[:, 0, :, 0] = 2.0 * (w - 1 - xs[:, 0])           # column 0 lands exactly on the last column at t = 0.5 ...
    fwd[:, 1, :, 0] = 0.0
    bwd[:, 1, :, w - 1] = 2.0 * (h - 1 - ys[:, w - 1])   # ... and the last column exactly on the last row
    bwd[:, 0, :, w - 1] = 0.0
    fwd, bwd, weight = iu.bad_inputs(fwd, bwd, seed + 1)
    _, _, weight_b = iu.bad_inputs(fwd, bwd, seed + 2)
    return fwd.contiguous(), bwd.contiguous(), weight, weight_b


_cache = {}


def case(b, h, w, k, kind):
    """Inputs and every host result of a case: made once, never written."""
    key = (b, h, w, k, kind)
    if key not in _cache:
        fwd, bwd, wf, wb = make_flows(b, h, w, kind)
        t = interp._times32(TIMES[k])
        t1 = np.float32(1.0) - t
        img0, img1 = iu.texture(b, h, w, 7 * h + w), iu.texture(b, h, w, 7 * h + w + 1)
        occ_f, occ_b = iu.masks(b, h, w, 7 * h + w + 2)
        thr = interp._hole_threshold(1.0 / 256)
        acc_w = torch.stack([interp.splat_accumulate_host(fwd, t, wf), interp.splat_accumulate_host(bwd, t1, wb)], 0)
        acc = torch.stack([interp.splat_accumulate_host(fwd, t), interp.splat_accumulate_host(bwd, t1)], 0)
        _cache[key] = dict(fwd=fwd, bwd=bwd, wf=wf, wb=wb, t=t, t1=t1, img0=img0, img1=img1, occ_f=occ_f, occ_b=occ_b, acc_w=acc_w,
                           acc=acc, avg_w=[interp.splat_normalize_host(a, thr) for a in acc_w],
                           frames={(layout, masked): interp.synthesize_host(
                               *((img0, img1) if layout == 'u8' else (iu.as_float_layout(img0), iu.as_float_layout(img1))), acc[0], acc[1], t,
                               occ_f if masked else None, occ_b if masked else None) for layout in ('u8', 'f32') for masked in (False, True)})
    return _cache[key]


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize('b,h,w,k,kind', CASES, ids=IDS)
def test_splat_is_the_restatement_bitwise(b, h, w, k, kind):
    c = case(b, h, w, k, kind)
    runs = [interp.splat_accumulators(dev(c['fwd']), c['t'], dev(c['bwd']), c['t1'], dev(c['wf']), dev(c['wb']), normalize=True)
            for _ in range(2)]
    acc, avg, hole = runs[0]
    assert acc.dtype == torch.int64 and tuple(acc.shape) == (2, b, k, 3, h, w)
    assert torch.equal(acc.cpu(), c['acc_w'])                                           # S_w, S_u, S_v of both directions
    for d in range(2):
        want_avg, want_hole = c['avg_w'][d]
        assert torch.equal(avg[d].cpu(), want_avg) and torch.equal(hole[d].cpu().bool(), want_hole), d
    assert all(torch.equal(p, q) for p, q in zip(runs[0], runs[1]))                     # two runs: the same bits
    if kind == 'converge':                                                              # every pixel of an image added to one word
        at = c['acc_w'][0, 0, TIMES[k].index(0.5), 0, h // 2, w // 2]
        assert int(at) == h * w * 65536
    # the public function: one direction, with and without weights
    flow, holes = interp.splat_flow(dev(c['fwd']), TIMES[k], weight=dev(c['wf']))
    assert torch.equal(flow.cpu(), c['avg_w'][0][0]) and torch.equal(holes.cpu(), c['avg_w'][0][1])
    assert torch.isfinite(flow).all()
    plain, _, _ = interp.splat_accumulators(dev(c['fwd']), c['t'])
    assert torch.equal(plain.cpu()[0], c['acc'][0])


@pytest.mark.parametrize('b,h,w,k,kind', CASES, ids=IDS)
def test_frames_are_the_restatement_bitwise(b, h, w, k, kind):
    c = case(b, h, w, k, kind)
    for layout in ('u8', 'f32'):
        i0, i1 = (c['img0'], c['img1']) if layout == 'u8' else (iu.as_float_layout(c['img0']), iu.as_float_layout(c['img1']))
        for masked in (False, True):
            kw = dict(occ_fwd=dev(c['occ_f']), occ_bwd=dev(c['occ_b'])) if masked else {}
            got, holes = interp.interpolate_frames(dev(i0), dev(i1), dev(c['fwd']), dev(c['bwd']), TIMES[k], return_holes=True, **kw)
            want, want_holes = c['frames'][(layout, masked)]
            assert got.dtype == torch.uint8 and tuple(got.shape) == (b, k, h, w, 3)
            assert torch.equal(got.cpu(), want), (layout, masked, int((got.cpu() != want).sum()))
            assert torch.equal(holes.cpu(), want_holes)
            alone = interp.interpolate_frames(dev(i0), dev(i1), dev(c['fwd']), dev(c['bwd']), TIMES[k], **kw)      # no hole output
            assert torch.equal(alone, got)


@pytest.mark.parametrize('b,h,w', SHAPES, ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_warp_is_the_restatement_bitwise(b, h, w):
    c = case(b, h, w, 1, 'mixed')
    f32 = iu.as_float_layout(c['img0'])
    images = {'u8': c['img0'], 'f32-3': f32, 'f32-1': f32[:, :1].contiguous(), 'f32-5': torch.cat([f32, f32[:, :2] * 0.37 - 3.0], 1).contiguous()}
    for flow in (c['fwd'], c['bwd']):
        for name, image in images.items():
            for padding in ('zeros', 'border'):
                want, want_mask = interp.backward_warp_host(image, flow, padding, True)
                got, mask = interp.backward_warp(dev(image), dev(flow), padding=padding, return_mask=True)
                assert got.dtype == image.dtype and torch.equal(got.cpu(), want), (name, padding)
                assert mask.dtype == torch.bool and torch.equal(mask.cpu(), want_mask)
                assert torch.equal(interp.backward_warp(dev(image), dev(flow), padding=padding), got)             # no mask output


@pytest.mark.parametrize('b,h,w', SHAPES, ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_memory_contract(b, h, w):
    """Red zones intact, inputs unchanged, and results independent of what the accumulators and the outputs held before (the entry
    point clears its workspace; every output element is written) -- with the optional outputs and inputs, and without them."""
    k = 3
    c = case(b, h, w, k, 'mixed')

    def run(_, g):
        fwd, bwd, wf = g.place(c['fwd']), g.place(c['bwd']), g.place(c['wf'])
        out = []
        for i0, i1 in ((c['img0'], c['img1']), (iu.as_float_layout(c['img0']), iu.as_float_layout(c['img1']))):
            i0, i1 = g.place(i0), g.place(i1)
            out += list(interp.backward_warp(i1, fwd, return_mask=True)) + [interp.backward_warp(i1, fwd, padding='border')]
            out += list(interp.interpolate_frames(i0, i1, fwd, bwd, TIMES[k], occ_fwd=g.place(c['occ_f']), occ_bwd=g.place(c['occ_b']),
                                                  return_holes=True))
            out.append(interp.interpolate_frames(i0, i1, fwd, bwd, TIMES[k]))
        out += list(interp.splat_flow(fwd, TIMES[k], weight=wf)) + list(interp.splat_flow(bwd, TIMES[k]))
        out += [t for t in interp.splat_accumulators(fwd, c['t'], bwd, c['t1'], wf, None) if t is not None]
        return out

    first = mg.contract(run, lambda guard: (guard,), device=DEV)
    assert first is not None
    assert any('interp.py' in site for site in mg.contract.last_sites)
    assert not [s for s in mg.contract.last_passed_through if 'interp.py' in s]


def test_argument_errors():
    """Every bad argument returns UM_ERR_BAD_ARG (-1) with a message that names the entry point, and launches nothing."""
    lib = _abi.load()
    h, w, k = 8, 8, 2
    flow = torch.zeros(1, 2, h, w, device=DEV)
    img = torch.zeros(1, h, w, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, k, h, w, 3, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(2 * k * 3 * h * w, dtype=torch.int64, device=DEV)
    times = (ctypes.c_float * (2 * 17))(*([0.5] * 34))
    f, i, o, a, n = flow.data_ptr(), img.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8
    s = torch.cuda.current_stream().cuda_stream

    def err():
        return lib.um_last_error_string()
    assert lib.um_image_warp(None, 1, f, o, None, 1, 3, h, w, 0, s) == -1 and b'um_image_warp' in err()
    assert lib.um_image_warp(i, 1, None, o, None, 1, 3, h, w, 0, s) == -1
    assert lib.um_image_warp(i, 1, f, None, None, 1, 3, h, w, 0, s) == -1
    assert lib.um_image_warp(i, 1, f, o, None, 1, 3, 1, w, 0, s) == -1
    assert lib.um_flow_splat(None, f, None, None, times, 1, k, h, w, 0.0, None, None, a, n, s) == -1 and b'um_flow_splat' in err()
    assert lib.um_flow_splat(f, f, None, None, times, 1, k, h, w, 0.0, None, None, None, n, s) == -1
    assert lib.um_flow_splat(f, f, None, None, times, 1, k, 1, w, 0.0, None, None, a, n, s) == -1 and b'h=1' in err()
    assert lib.um_flow_splat(f, f, None, None, times, 1, 17, h, w, 0.0, None, None, a, n, s) == -1 and b'k=17' in err()
    assert lib.um_flow_splat(f, f, None, None, times, 1, k, 1024, 2049, 0.0, None, None, a, 1 << 40, s) == -1 and b'2^21' in err()
    assert lib.um_flow_splat(f, f, None, None, times, 1, k, h, w, 0.0, None, None, a, n - 8, s) == -1 and b'needed' in err()
    assert lib.um_frame_synthesize(None, i, 1, None, None, times, a, n, o, None, 1, k, h, w, 0.0, s) == -1 and b'um_frame_synthesize' in err()
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, None, n, o, None, 1, k, h, w, 0.0, s) == -1
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, a, n, None, None, 1, k, h, w, 0.0, s) == -1
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, a, n, o, None, 1, k, 1, w, 0.0, s) == -1
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, a, n, o, None, 1, 17, h, w, 0.0, s) == -1
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, a, 1 << 40, o, None, 1, k, 2048, 1025, 0.0, s) == -1
    assert lib.um_frame_synthesize(i, i, 1, None, None, times, a, n - 8, o, None, 1, k, h, w, 0.0, s) == -1 and b'needed' in err()
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(ws.any())                                    # nothing was launched
    with pytest.raises(ValueError, match='um_flow_splat|2\\^21'):
        interp.splat_flow(torch.zeros(1, 2, 2048, 1025, device=DEV), [0.5])


def test_forward_sequence_interpolate_on_the_device():
    from unimatch_amd import UniMatch
    from unimatch_amd.synth import CONFIGS, synth_frames, synth_state_dict
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    frames = synth_frames(4, 64, 96, seed=2301).to(DEV)
    plain = model.forward_sequence(frames, pred_bidir_flow=True, consistency_check=True, pairs_per_launch=2, **kw)
    out = model.forward_sequence(frames, pred_bidir_flow=True, pairs_per_launch=2, interpolate=2, **kw)
    assert torch.equal(out['flow'], plain['flow']) and torch.equal(out['flow_bwd'], plain['flow_bwd'])
    assert set(out) == {'flow', 'flow_bwd', 'frames_between', 'carry'}
    want = interp.interpolate_frames(frames[:-1].contiguous(), frames[1:].contiguous(), plain['flow'], plain['flow_bwd'], [1 / 3, 2 / 3],
                                     occ_fwd=plain['occ_fwd'], occ_bwd=plain['occ_bwd'])
    assert out['frames_between'].dtype == torch.uint8 and tuple(out['frames_between'].shape) == (3, 2, 64, 96, 3)
    assert torch.equal(out['frames_between'], want)
    host = interp.interpolate_frames(frames[:-1].cpu().contiguous(), frames[1:].cpu().contiguous(), plain['flow'].cpu(),
                                     plain['flow_bwd'].cpu(), [1 / 3, 2 / 3], occ_fwd=plain['occ_fwd'].cpu(), occ_bwd=plain['occ_bwd'].cpu())
    assert torch.equal(want.cpu(), host)
    again = model.forward_sequence(frames, pred_bidir_flow=True, consistency_check=True, pairs_per_launch=2, interpolate=0, **kw)
    assert set(again) == set(plain) and all(torch.equal(again[key], plain[key]) for key in plain if key != 'carry')
