"""GPU tests of the stereo inference path: ``um_image_prepare_flip`` / ``um_pred_restore_flip`` against ``torch.flip`` of what the
unflipped entry points write (bit for bit: the mirror is an index remap with the mirrored column's arithmetic), ``out=`` into the
halves of a doubled batch, and ``UniMatch.predict(pred_right_disp / pred_bidir_disp)`` against the manual ``torch.flip`` /
``torch.cat`` composition of the reference's lines (evaluate_stereo.py:790-841) around ``model(...)``, without host synchronisation."""
import ctypes

import pytest
import torch

from unimatch_amd import UniMatch, _abi, prepost
from unimatch_amd.ops import KernelTimer
from unimatch_amd.prepost import InferenceGeometry
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(37, 53), (64, 96), (5, 1), (1, 7)]


def frames(b, h, w, seed, u8=True):
    x = torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return x if u8 else x.permute(0, 3, 1, 2).float().contiguous()


def geometries(h, w):
    for transpose in (False, True):
        yield InferenceGeometry.padded((h, w), 'sintel', 32, transpose=transpose)
        yield InferenceGeometry.resized((h, w), (64, 96), transpose=transpose)    # 16-byte stores
        yield InferenceGeometry.resized((h, w), (45, 67), transpose=transpose)    # scalar stores
    yield InferenceGeometry.resized((h, w), (h, w))                                # nothing to do but the mirror


def old_prepare(x, geom, mean=None, std=None):
    """The existing entry point ``um_image_prepare`` itself, through ctypes."""
    u8 = x.dtype == torch.uint8
    b, (h, w) = x.shape[0], prepost.image_size(x)
    out = torch.empty((b, 3) + geom.size, dtype=torch.float32, device=x.device)
    fm = (ctypes.c_float * 3)(*mean) if mean else None
    fs = (ctypes.c_float * 3)(*std) if std else None
    _abi.check(_abi.load().um_image_prepare(x.data_ptr(), 1 if u8 else 0, out.data_ptr(), b, h, w, int(geom.transpose), fm, fs,
                                            1 if geom.mode == 'resize' else 0, geom.size[0], geom.size[1], geom.crop[0], geom.crop[1],
                                            torch.cuda.current_stream().cuda_stream), 'um_image_prepare')
    return out


def old_restore(pred, geom, kind):
    b, c, hp, wp = pred.shape
    h, w = geom.shape
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=pred.device)
    _abi.check(_abi.load().um_pred_restore(pred.data_ptr(), out.data_ptr(), b, c, hp, wp, 1 if geom.mode == 'resize' else 0, geom.crop[0],
                                           geom.crop[1], h, w, {'flow': 0, 'disparity': 1, 'depth': 2}[kind], int(geom.transpose),
                                           torch.cuda.current_stream().cuda_stream), 'um_pred_restore')
    return out


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('u8', [True, False])
def test_image_prepare_flip_is_flip_of_the_unflipped_entry_point(h, w, u8):
    x = frames(2, h, w, seed=h * 100 + w, u8=u8).to(DEV)
    ops = prepost._hip()
    for geom in geometries(h, w):
        for normalize in (False, True):
            mean, std = (prepost.IMAGENET_MEAN, prepost.IMAGENET_STD) if normalize else (None, None)
            plain = old_prepare(x, geom, mean, std)
            args = (x, geom.size, geom.mode, geom.crop, geom.transpose, mean, std)
            assert torch.equal(ops.image_prepare(*args, hflip=False), plain), geom              # hflip = 0 is the old entry point
            got = ops.image_prepare(*args, hflip=True)
            assert torch.equal(got, torch.flip(plain, [-1])), (geom, normalize)
            assert torch.equal(geom.prepare(x, normalize=normalize, hflip=True)[0], got)
            assert torch.equal(got.cpu(), geom.prepare(x.cpu(), normalize=normalize, hflip=True)[0])   # and the host restatement
            # out=: the second half of a doubled batch, the first half left untouched
            both = torch.full((4, 3) + geom.size, -7.0, device=DEV)
            back = geom.prepare(x, normalize=normalize, hflip=True, out=both[2:])[0]
            assert back.data_ptr() == both[2:].data_ptr() and torch.equal(both[2:], got) and (both[:2] == -7.0).all()
            geom.prepare(x, normalize=normalize, out=both[:2])
            assert torch.equal(both[:2], plain) and torch.equal(both[2:], got)
    with pytest.raises(ValueError):
        geom.prepare(x, out=torch.zeros(1, 3, h, w, device=DEV))
    with pytest.raises(ValueError):
        ops.image_prepare(x, (h, w), out=torch.zeros(2, 3, h, w))


@pytest.mark.parametrize('h,w', SIZES)
def test_pred_restore_flip_is_flip_of_the_unflipped_entry_point(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    ops = prepost._hip()
    for geom in geometries(h, w):
        flow = (torch.randn(2, 2, *geom.size, generator=g) * 30).to(DEV)
        for kind, pred in (('flow', flow), ('disparity', flow[:, :1].abs().contiguous()), ('depth', flow[:, 1:].abs().contiguous() + 0.1)):
            plain = old_restore(pred, geom, kind)
            args = (pred, geom.shape, geom.mode, geom.crop, kind, geom.transpose)
            assert torch.equal(ops.pred_restore(*args, hflip=False), plain), (geom, kind)
            got = ops.pred_restore(*args, hflip=True)
            assert torch.equal(got, torch.flip(plain, [-1])), (geom, kind)
            assert torch.equal(geom.restore(pred, kind, hflip=True), got)
            assert torch.equal(got.cpu(), geom.restore(pred.cpu(), kind, hflip=True))
            both = torch.full((4,) + tuple(plain.shape[1:]), -7.0, device=DEV)
            back = geom.restore(pred, kind, hflip=True, out=both[2:])
            assert back.data_ptr() == both[2:].data_ptr() and torch.equal(both[2:], got) and (both[:2] == -7.0).all()
            geom.restore(pred, kind, out=both[:2])
            assert torch.equal(both[:2], plain)
        sq = geom.restore(flow[:, 0].contiguous(), 'disparity', hflip=True)                     # [B, hp, wp] in, [B, H, W] out
        assert torch.equal(sq, torch.flip(old_restore(flow[:, :1].contiguous(), geom, 'disparity'), [-1])[:, 0])


# ------------------------------------------------------------------ predict
_model = {}


def stereo_model():
    if not _model:
        ck, fk = CONFIGS['gmstereo_s1']
        model = UniMatch(**ck).eval()
        model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
        _model['m'] = (model.to(DEV), dict(fk))
    return _model['m']


def manual_views(model, geom, left, right, kw, right_disp, bidir):
    """evaluate_stereo.py:790-841 written out with torch.flip / torch.cat around ``model(...)``."""
    a, b = geom.prepare(left, right)
    if bidir:
        a, b = torch.cat((a, torch.flip(b, [-1])), 0), torch.cat((b, torch.flip(a, [-1])), 0)
    if right_disp:
        a, b = torch.flip(b, [-1]).contiguous(), torch.flip(a, [-1]).contiguous()
    pred = geom.restore(model(a, b, **kw)['flow_preds'][-1], 'disparity')
    if right_disp:
        pred = torch.flip(pred, [-1])
    if bidir:                                                   # the caller's flip-back of the second half (:833-834)
        n = pred.shape[0] // 2
        pred = torch.cat((pred[:n], torch.flip(pred[n:], [-1])), 0)
    return pred


@pytest.mark.parametrize('batch,h,w,size', [(2, 64, 96, None), (1, 37, 53, (64, 64))])
@pytest.mark.parametrize('right_disp,bidir', [(True, False), (False, True), (True, True)])
def test_predict_stereo_views_equal_the_manual_composition_and_never_synchronise(batch, h, w, size, right_disp, bidir):
    model, kw = stereo_model()
    left, right = (x.to(DEV) for x in synth_images(batch, h, w, seed=1000, kind='shift', normalized=True))
    geom = prepost.geometry_for((h, w), size, 32, 'sintel')
    views = dict(inference_size=size, pred_right_disp=right_disp, pred_bidir_disp=bidir)
    with torch.no_grad():
        want = manual_views(model, geom, left, right, kw, right_disp, bidir)
        first = model.predict(left, right, **views, **kw)['flow_preds'][-1]         # allocator, weight planes warm
        torch.cuda.synchronize()
        ops = prepost._hip()
        ops.timer = KernelTimer()
        torch.cuda.set_sync_debug_mode('error')
        try:
            got = model.predict(left, right, **views, **kw)['flow_preds'][-1]
            records = [r[0] for r in ops.timer.records]
        finally:
            torch.cuda.set_sync_debug_mode('default')
            ops.timer = None
    assert got.shape == ((2 if bidir else 1) * batch, h, w) and torch.isfinite(got).all()
    assert torch.equal(got, want) and torch.equal(first, got)
    # at most four prepares into two preallocated tensors and two restores; an unresized, unmirrored half still costs its copy
    assert records == (['image_prepare'] * 4 + ['pred_restore'] * 2 if bidir else ['image_prepare'] * 2 + ['pred_restore'])
    with torch.no_grad():
        plain = model.predict(left, right, inference_size=size, **kw)['flow_preds'][-1]
    assert not torch.equal(got[:batch] if right_disp else got[-batch:], plain)
    model.check_operand_range()


def test_predict_refuses_stereo_views_for_other_tasks():
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval().to(DEV)
    i0, i1 = (x.to(DEV) for x in synth_images(1, 64, 96, seed=1000, kind='shift'))
    for views in (dict(pred_right_disp=True), dict(pred_bidir_disp=True)):
        with pytest.raises(ValueError):
            model.predict(i0, i1, **views, **fk)
