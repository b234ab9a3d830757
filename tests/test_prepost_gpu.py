"""GPU tests of the inference-size handling: ``um_image_prepare`` / ``um_pred_restore`` against the host restatement bit for bit
(every source layout x sizing mode x transpose x normalisation, every prediction kind x sizing mode x transpose, at odd and at
evaluation sizes) and against ``F.interpolate`` on the CPU to ``4 * 2^-23 * max|input|`` (the bound of test_prepost_cpu.py: the same
fp32 weights, at most seven fp32 operations in another order), no host synchronisation, determinism, ``UniMatch.predict`` end to end
and the stereo / depth validation loops."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unimatch_amd import UniMatch, evaluate, io, metrics, prepost
from unimatch_amd.ops import KernelTimer
from unimatch_amd.prepost import InferenceGeometry
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_images, synth_state_dict
from tests.metrics_util import SHARE_KEYS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP4 = 4 * 2.0 ** -23
MEAN, STD = (torch.tensor(c).view(1, 3, 1, 1) for c in (prepost.IMAGENET_MEAN, prepost.IMAGENET_STD))
# (batch, H, W, resize targets): 53 and 1242 are no multiples of 4 (scalar stores), 45 x 67 is an unaligned target
CASES = [(3, 37, 53, ((64, 96), (45, 67))), (1, 375, 1242, ((384, 1248),)), (3, 375, 1242, ((384, 1248),)), (1, 1080, 1920, ((768, 1344),))]


def frames(b, h, w, seed):
    return torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def geometries(h, w, sizes, transpose):
    yield 'pad', InferenceGeometry.padded((h, w), 'sintel', 32, transpose=transpose)
    for size in sizes:
        yield 'resize', InferenceGeometry.resized((h, w), size, transpose=transpose)


# ------------------------------------------------------------------ 1, 2. the kernels against the restatement and F.interpolate
@pytest.mark.parametrize('b,h,w,sizes', CASES)
@pytest.mark.parametrize('transpose', [False, True])
def test_image_prepare_against_restatement_and_interpolate(b, h, w, sizes, transpose):
    u = frames(b, h, w, seed=h + b)
    f = u.permute(0, 3, 1, 2).float().contiguous()
    for mode, geom in geometries(h, w, sizes, transpose):
        for layout, x in (('u8', u), ('f32', f)):
            for normalize in (False, True):
                got = geom.prepare(x.to(DEV), normalize=normalize)[0]
                want = geom.prepare(x, normalize=normalize)[0]
                tag = f'{b}x{h}x{w} {layout} {mode} -> {geom.size} transpose={transpose} normalize={normalize}'
                assert got.is_cuda and got.shape == want.shape == (b, 3) + geom.size and got.dtype == torch.float32, tag
                assert torch.equal(got.cpu(), want), (tag, (got.cpu() - want).abs().max().item())
                if mode == 'resize':
                    t = f.transpose(-2, -1) if transpose else f
                    t = (t / 255 - MEAN) / STD if normalize else t
                    ref = F.interpolate(t, size=geom.size, mode='bilinear', align_corners=True)
                    err, bound = (got.cpu() - ref).abs().max().item(), ULP4 * t.abs().max().item()
                    print(f'prepare {tag}: max |kernel - F.interpolate| = {err:.3g} (bound {bound:.3g})')
                    assert err <= bound, tag


@pytest.mark.parametrize('b,h,w,sizes', CASES)
@pytest.mark.parametrize('transpose', [False, True])
def test_pred_restore_against_restatement_and_interpolate(b, h, w, sizes, transpose):
    g = torch.Generator().manual_seed(h + 7 * b)
    for mode, geom in geometries(h, w, sizes, transpose):
        flow = torch.randn(b, 2, *geom.size, generator=g) * 40
        for kind, pred in (('flow', flow), ('disparity', flow[:, 0].abs().contiguous()), ('depth', flow[:, 1:].abs().contiguous() + 0.1)):
            got = geom.restore(pred.to(DEV), kind)
            want = geom.restore(pred, kind)
            tag = f'{b}x{h}x{w} {kind} {mode} {geom.size} -> back, transpose={transpose}'
            assert got.is_cuda and got.shape == want.shape == pred.shape[:-2] + (h, w), tag
            assert torch.equal(got.cpu(), want), (tag, (got.cpu() - want).abs().max().item())
            if mode == 'resize':                                       # the reference's lines on the CPU
                ih, iw = geom.image_size
                p4 = pred if pred.dim() == 4 else pred.unsqueeze(1)
                ref = F.interpolate(p4, size=(ih, iw), mode='bilinear', align_corners=True)
                factor = 1.0
                if kind == 'flow':
                    ref[:, 0] = ref[:, 0] * iw / geom.size[-1]
                    ref[:, 1] = ref[:, 1] * ih / geom.size[-2]
                    factor = max(iw / geom.size[-1], ih / geom.size[-2], 1.0)
                elif kind == 'disparity':
                    ref = ref * iw / float(geom.size[-1])
                    factor = max(iw / geom.size[-1], 1.0)
                ref = ref.transpose(-2, -1) if transpose else ref
                ref = ref if pred.dim() == 4 else ref.squeeze(1)
                err, bound = (got.cpu() - ref).abs().max().item(), ULP4 * pred.abs().max().item() * factor
                print(f'restore {tag}: max |kernel - torch ops| = {err:.3g} (bound {bound:.3g})')
                assert err <= bound, tag


def test_identity_makes_no_launch():
    x = torch.rand(2, 3, 64, 96, device=DEV)
    geom = InferenceGeometry.padded(x.shape, 'sintel', 32)
    ops = prepost._hip()
    ops.timer = KernelTimer()
    try:
        assert geom.prepare(x)[0] is x and geom.restore(x[:, :2], 'flow').data_ptr() == x.data_ptr()
        assert InferenceGeometry.resized(x.shape, (64, 96)).prepare(x)[0] is x
        assert ops.timer.records == []
        assert geom.prepare(x, normalize=True)[0] is not x and len(ops.timer.records) == 1       # normalising is work
    finally:
        ops.timer = None


# ------------------------------------------------------------------ 3, 4. no synchronisation, determinism
def flow_model():
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    return model.to(DEV), {k: v for k, v in fk.items()}


def test_prepare_restore_and_predict_never_synchronise():
    """torch's synchronisation debug mode raises on any device-to-host copy or stream wait; the launch census of ``KernelTimer``
    shows one ``image_prepare`` per image and one ``pred_restore`` per prediction."""
    u0, u1 = frames(2, 125, 189, seed=1).to(DEV), frames(2, 125, 189, seed=2).to(DEV)
    tall = frames(1, 189, 125, seed=3).to(DEV)
    model, kw = flow_model()
    geom = InferenceGeometry.resized((125, 189), (128, 192))
    tgeom = InferenceGeometry.nearest((189, 125), 32)
    pred = torch.randn(2, 2, 128, 192, device=DEV)

    def work():
        a, b = geom.prepare(u0, u1)
        c, = geom.prepare(u0, normalize=True)
        r = geom.restore(pred, 'flow')
        d, = tgeom.prepare(tall)
        e = tgeom.restore(pred[:1], 'flow')
        p = model.predict(u0, u1, inference_size=(128, 192), **kw)['flow_preds'][-1]
        q = model.predict(u0.permute(0, 3, 1, 2).float(), u1.permute(0, 3, 1, 2).float(), **kw)['flow_preds'][-1]
        return a, b, c, r, d, e, p, q

    first = work()                                                      # library, allocator, weight planes warm
    torch.cuda.synchronize()
    ops = prepost._hip()
    ops.timer = KernelTimer()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                             # the mode does catch a synchronising call
        second = work()
        records = [r[0] for r in ops.timer.records]
    finally:
        torch.cuda.set_sync_debug_mode('default')
        ops.timer = None
    assert records == ['image_prepare'] * 3 + ['pred_restore', 'image_prepare', 'pred_restore'] + \
        ['image_prepare'] * 2 + ['pred_restore'] + ['image_prepare'] * 2 + ['pred_restore']
    torch.cuda.synchronize()
    for a, b in zip(first, second):                                      # and two calls give equal bits
        assert torch.equal(a, b)
    assert first[6].shape == first[7].shape == (2, 2, 125, 189) and first[5].shape == (1, 2, 189, 125)
    model.check_operand_range()


def test_two_calls_give_equal_bits_whatever_ran_between():
    u = frames(2, 375, 1242, seed=9).to(DEV)
    geom = InferenceGeometry.resized((375, 1242), (384, 1248))
    other = InferenceGeometry.padded((37, 53), 'kitti', 32, transpose=True)
    pred = torch.randn(2, 1, 384, 1248, device=DEV)
    a, r = geom.prepare(u, normalize=True)[0], geom.restore(pred, 'disparity')
    other.prepare(frames(1, 37, 53, seed=1).to(DEV))
    other.restore(torch.randn(1, 2, *other.size, device=DEV), 'flow')
    assert torch.equal(geom.prepare(u, normalize=True)[0], a) and torch.equal(geom.restore(pred, 'disparity'), r)


# ------------------------------------------------------------------ 5. the model end to end
def build(name, h, w, batch=1):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    i0, i1 = synth_images(batch, h, w, seed=1000, kind='shift', normalized=(fk['task'] != 'flow'))
    kw = dict(fk)
    if fk['task'] == 'depth':
        k, pose = synth_camera(batch, h, w)
        kw.update(intrinsics=k.to(DEV), pose=pose.to(DEV))
    return model.to(DEV), i0.to(DEV), i1.to(DEV), kw


def torch_restore(pred, size, task, inference_size):
    """The reference's resize-back lines (evaluate_flow.py:751-755, evaluate_stereo.py:373-375, evaluate_depth.py:128-131)."""
    if task == 'flow':
        out = F.interpolate(pred, size=size, mode='bilinear', align_corners=True)
        out[:, 0] = out[:, 0] * size[-1] / inference_size[-1]
        out[:, 1] = out[:, 1] * size[-2] / inference_size[-2]
        return out
    out = F.interpolate(pred.unsqueeze(1), size=size, mode='bilinear', align_corners=True).squeeze(1)
    return out * size[-1] / float(inference_size[-1]) if task == 'stereo' else out


@pytest.mark.parametrize('name,padded,resized', [('gmflow_s1', (59, 90), ((127, 191), (64, 96))),
                                                 ('gmstereo_s1', (59, 90), ((127, 191), (64, 96))),
                                                 ('gmdepth_s1', (90, 120), ((191, 255), (96, 128)))])
def test_predict_end_to_end(name, padded, resized):
    """``predict`` against the torch-op pipeline around ``model(...)``, to ``4 * 2^-23 * max|prediction|`` times the restore factor.
    That bound is the restore's; the model amplifies an input difference of one ulp by a factor nobody has bounded, so it can only
    be asserted between pipelines that hand the model the same bits.  Three cases:

      padded            padding copies values: the pipelines are ``InputPadder.pad`` -> model -> ``unpad`` and ``predict``.
      resized, exact    sizes with ``(in - 1) = 2 (out - 1)``: the source coordinate ``2 dst`` is exact, the weights are 1 and 0, so
                        ``F.interpolate`` and the kernel pick the same pixels bit for bit (asserted); everything is torch ops.
      resized, general  fractional weights (59 x 90 -> 64 x 96, 90 x 120 -> 96 x 128).  The prepared pair is asserted to lie within
                        ``4 * 2^-23 * max|x|`` of ``F.interpolate``; the model is then given that prepared pair on both sides, and
                        ``predict`` is asserted against the torch resize-back and rescale of that prediction.  The figure of the
                        all-torch pipeline, whose model input differs by that rounding, is printed beside it (observed on an MI355X:
                        6.7e-6 at max|flow| 3.1, 9.5e-6 at max|disparity| 21, 2.6e-6 at max|depth| 6.2)."""
    task = CONFIGS[name][1]['task']
    factor, mode = {'flow': (8, 'sintel'), 'stereo': (32, 'sintel'), 'depth': (16, 'kitti')}[task]
    # padded
    model, i0, i1, kw = build(name, *padded)
    padder = io.InputPadder(i0.shape, mode=mode, padding_factor=factor)
    a, b = padder.pad(i0, i1)
    want = padder.unpad(model(a, b, **kw)['flow_preds'][-1])
    got = model.predict(i0, i1, **kw)['flow_preds'][-1]
    err = (got - want).abs().max().item()
    print(f'{name} padded {padded}: max |predict - torch ops| = {err:.3g}')
    assert got.shape == want.shape and got.shape[-2:] == padded and err <= ULP4 * want.abs().max().item()
    # resized, exact weights
    (h, w), size = resized
    model, i0, i1, kw = build(name, h, w)
    a, b = (F.interpolate(x, size=size, mode='bilinear', align_corners=True) for x in (i0, i1))
    mine = InferenceGeometry.resized((h, w), size).prepare(i0, i1)
    assert torch.equal(mine[0], a) and torch.equal(mine[1], b) and torch.equal(a, i0[:, :, ::2, ::2])
    pred = model(a, b, **kw)['flow_preds'][-1]
    got = model.predict(i0, i1, inference_size=size, **kw)['flow_preds'][-1]
    scale = max(w / size[1], h / size[0], 1.0) if task != 'depth' else 1.0
    bound = ULP4 * pred.abs().max().item() * scale
    want = torch_restore(pred.cpu(), (h, w), task, size)
    err = (got.cpu() - want).abs().max().item()
    on_device = (got - torch_restore(pred.clone(), (h, w), task, size)).abs().max().item()
    print(f'{name} resized {(h, w)} -> {size}: max |predict - torch ops| = {err:.3g} with the CPU ops, {on_device:.3g} with the '
          f'device ops (bound {bound:.3g})')
    assert got.shape == want.shape and got.shape[-2:] == (h, w) and err <= bound
    # resized, fractional weights
    h, w = padded
    model, i0, i1, kw = build(name, h, w)
    mine = InferenceGeometry.resized((h, w), size).prepare(i0, i1)
    for x, m in zip((i0, i1), mine):                           # the kernel's resize against F.interpolate on the CPU
        ref = F.interpolate(x.cpu(), size=size, mode='bilinear', align_corners=True)
        err, bound = (m.cpu() - ref).abs().max().item(), ULP4 * x.abs().max().item()
        print(f'{name} prepare {(h, w)} -> {size}: max |kernel - F.interpolate| = {err:.3g} (bound {bound:.3g})')
        assert err <= bound
    pred = model(mine[0], mine[1], **kw)['flow_preds'][-1]     # the same prepared pair on both sides
    got = model.predict(i0, i1, inference_size=size, **kw)['flow_preds'][-1]
    scale = max(w / size[1], h / size[0], 1.0) if task != 'depth' else 1.0
    bound = ULP4 * pred.abs().max().item() * scale
    err = (got.cpu() - torch_restore(pred.cpu(), (h, w), task, size)).abs().max().item()
    a, b = (F.interpolate(x, size=size, mode='bilinear', align_corners=True) for x in (i0, i1))
    loose = model(a, b, **kw)['flow_preds'][-1]
    diff = (got.cpu() - torch_restore(loose.cpu(), (h, w), task, size)).abs().max().item()
    print(f'{name} resized {(h, w)} -> {size}: max |predict - torch resize-back of the same prediction| = {err:.3g} (bound {bound:.3g}); '
          f'against the all-torch pipeline, whose model input differs by rounding: {diff:.3g} at max |prediction| = '
          f'{pred.abs().max().item():.3g}')
    assert got.shape[-2:] == (h, w) and err <= bound
    model.check_operand_range()


# ------------------------------------------------------------------ 6. the validation loops
def compare(res, want, prefix):
    for key, value in res.items():
        short = key[len(prefix):]
        short = {'3px': 'thres3'}.get(short, short)
        print(key, value, want[short])
        assert np.isfinite(value)
        if short in SHARE_KEYS:
            assert value == want[short], key
        else:
            assert abs(value - want[short]) <= 1e-12 * abs(want[short]), (key, value, want[short])


def by_hand(model, geom_case, a, b, task, kw):
    """The reference's block around the model for one sample, host tensors in, host prediction at the images' size out (or the padded
    prediction and its padder).  ``geom_case = (h, w, inference_size, independent)``.  ``independent``: torch ops only
    (``F.interpolate`` both ways and the rescale lines); used at sizes with ``(in - 1) = 2 (out - 1)``, where the resize weights are
    0, 1/2 and 1, every blend is one rounding whatever the order, and torch's values are the kernels' bit for bit.  Otherwise the
    host restatement prepares and restores, after being held to ``F.interpolate`` and the rescale lines within the 4-ulp bound here:
    torch's own resize would change the model's input by a rounding and the metrics by more than the 1e-12 that is asserted."""
    h, w, size, independent = geom_case
    if independent:
        a, b = (F.interpolate(x, size=size, mode='bilinear', align_corners=True) for x in (a, b))
    else:
        geom = InferenceGeometry.resized((h, w), size)
        pa, pb = geom.prepare(a, b)
        for x, m in ((a, pa), (b, pb)):
            assert (m - F.interpolate(x, size=size, mode='bilinear', align_corners=True)).abs().max() <= ULP4 * x.abs().max()
        a, b = pa, pb
    with torch.no_grad():
        pred = model(a.to(DEV), b.to(DEV), task=task, **kw)['flow_preds'][-1].cpu()
    back = torch_restore(pred, (h, w), task, size)
    if independent:
        return back
    mine = geom.restore(pred, 'disparity' if task == 'stereo' else 'depth')
    assert (mine - back).abs().max() <= ULP4 * pred.abs().max() * (max(w / size[1], 1.0) if task == 'stereo' else 1.0)
    return mine


@pytest.mark.parametrize('h,w,inference_size,independent', [(59, 90, None, True), (127, 191, (64, 96), True), (59, 90, (64, 96), False)])
def test_validate_stereo_end_to_end(h, w, inference_size, independent):
    """gmstereo_s1 over uint8 frames at odd sizes.  The model has no CPU backend, so "the CPU run" is this: the frames normalised and
    padded or resized by hand on the host, the model's outputs copied back, resized back by hand, and ``StereoMetrics`` fed on the
    host.  How the resized references are built: :func:`by_hand`."""
    ck, fk = CONFIGS['gmstereo_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    samples = []
    for seed in (700, 701, 702, 703):
        i0, i1 = synth_images(1, h, w, seed=seed, kind='shift')
        left, right = (x[0].permute(1, 2, 0).round().to(torch.uint8).contiguous() for x in (i0, i1))
        gt = torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) * 12
        gt[gt < 2] = 0
        samples.append((left, right, gt if seed != 702 else torch.zeros(h, w)))
    res = evaluate.validate_stereo(model, samples, 'syn', inference_size=inference_size, padding_factor=32, batch_size=1, **kw)
    ref = metrics.StereoMetrics()
    for left, right, gt in samples:
        a, b = ((x.permute(2, 0, 1)[None].float() / 255 - MEAN) / STD for x in (left, right))
        if inference_size is None:
            padder = io.InputPadder((h, w), padding_factor=32)
            a, b = padder.pad(a, b)
            with torch.no_grad():
                pred = model(a.to(DEV), b.to(DEV), task='stereo', **kw)['flow_preds'][-1]
            ref.update(pred.cpu(), gt[None], padder=padder)
        else:
            ref.update(by_hand(model, (h, w, inference_size, independent), a, b, 'stereo', kw), gt[None])
    want = ref.compute()
    assert want['skipped'] == 1 and set(res) == {'syn_epe', 'syn_d1', 'syn_3px'}
    compare(res, want, 'syn_')
    model.check_operand_range()


@pytest.mark.parametrize('h,w,inference_size,independent', [(90, 120, None, True), (191, 255, (96, 128), True),
                                                            (90, 120, (96, 128), False)])
def test_validate_depth_end_to_end(h, w, inference_size, independent):
    """gmdepth_s1; the reference is built as in :func:`test_validate_stereo_end_to_end` (host metrics of the device model's outputs)."""
    ck, fk = CONFIGS['gmdepth_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    k, pose = synth_camera(1, h, w)
    samples = []
    for seed in (800, 801, 802):
        i0, i1 = synth_images(1, h, w, seed=seed, kind='shift', normalized=True)
        g = torch.Generator().manual_seed(seed)
        depth = 0.3 + 11 * torch.rand(h, w, generator=g)
        valid = (torch.rand(h, w, generator=g) > 0.3).float()
        samples.append((i0[0], i1[0], k[0], pose[0], depth, valid if seed != 801 else torch.zeros(h, w)))
    assert (kw['min_depth'], kw['max_depth']) == (1 / 10., 1 / 0.5)          # the configuration's inverse-depth range
    res = evaluate.validate_depth(model, samples, 'syn', inference_size=inference_size, padding_factor=16, min_depth=0.5, max_depth=10.,
                                  **{k: v for k, v in kw.items() if k not in ('min_depth', 'max_depth')})
    ref = metrics.DepthMetrics(0.5, 10.)
    for i0, i1, ki, pi, depth, valid in samples:
        cam = dict(kw, intrinsics=ki[None].to(DEV), pose=pi[None].to(DEV))
        if inference_size is None:
            padder = io.InputPadder((h, w), mode='kitti', padding_factor=16)
            a, b = padder.pad(i0[None], i1[None])
            with torch.no_grad():
                pred = model(a.to(DEV), b.to(DEV), task='depth', **cam)['flow_preds'][-1]
            ref.update(pred.cpu(), depth[None], valid[None], padder=padder)
        else:
            ref.update(by_hand(model, (h, w, inference_size, independent), i0[None], i1[None], 'depth', cam), depth[None], valid[None])
    want = ref.compute()
    assert want['skipped'] == 1 and set(res) == {'syn_' + e for e in evaluate.DEPTH_ERRORS}
    compare(res, want, 'syn_')
    model.check_operand_range()
