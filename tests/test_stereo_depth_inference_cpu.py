"""CPU tests of the stereo / depth inference path: the horizontal mirror of ``InferenceGeometry.prepare`` / ``restore`` (host
restatement), ``UniMatch.predict(pred_right_disp / pred_bidir_disp)`` with the oracle injected as backend against the manual
``torch.flip`` / ``torch.cat`` composition of the reference's lines (evaluate_stereo.py:790-841), and the two directory runners on
temporary directories with a stand-in model."""
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, io, prepost, visualize
from unimatch_amd.prepost import InferenceGeometry
from unimatch_amd.synth import CONFIGS, synth_camera, synth_images, synth_state_dict
from tests.oracle_ops import OracleOps


def frames(b, h, w, seed, u8=True):
    x = torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return x if u8 else x.permute(0, 3, 1, 2).float().contiguous()


def geometries(h, w):
    yield InferenceGeometry.padded((h, w), 'sintel', 32)
    yield InferenceGeometry.padded((h, w), 'kitti', 16, transpose=True)
    yield InferenceGeometry.resized((h, w), (64, 96))
    yield InferenceGeometry.resized((h, w), (45, 67), transpose=True)
    yield InferenceGeometry.resized((h, w), (h, w))                              # nothing to do but the mirror


# ------------------------------------------------------------------ 1. the mirror is torch.flip of the unflipped result
@pytest.mark.parametrize('h,w', [(37, 53), (64, 96), (5, 1), (1, 7)])
@pytest.mark.parametrize('u8', [True, False])
def test_prepare_host_hflip_is_flip_of_the_unflipped_result(h, w, u8):
    x = frames(2, h, w, seed=h + w, u8=u8)
    for geom in geometries(h, w):
        for normalize in (False, True):
            plain = geom.prepare(x, normalize=normalize)[0]
            got = geom.prepare(x, normalize=normalize, hflip=True)[0]
            assert got.is_contiguous() and torch.equal(got, torch.flip(plain, [-1])), geom
            assert torch.equal(prepost.prepare_host(x, geom, hflip=True), torch.flip(prepost.prepare_host(x, geom), [-1]))
            # out=: the second half of a doubled batch, the first half left untouched
            both = torch.full((4, 3) + geom.size, -7.0)
            back = geom.prepare(x, normalize=normalize, hflip=True, out=both[2:])[0]
            assert back.data_ptr() == both[2:].data_ptr() and torch.equal(both[2:], got) and (both[:2] == -7.0).all()
            geom.prepare(x, normalize=normalize, out=both[:2])
            assert torch.equal(both[:2], plain) and torch.equal(both[2:], got)
    with pytest.raises(ValueError):
        geom.prepare(x, out=torch.zeros(1, 3, h, w))
    with pytest.raises(ValueError):
        geom.prepare(x, x, out=torch.zeros(2, 3, h, w))


@pytest.mark.parametrize('h,w', [(37, 53), (64, 96), (5, 1), (1, 7)])
def test_restore_host_hflip_is_flip_of_the_unflipped_result(h, w):
    g = torch.Generator().manual_seed(h * w)
    for geom in geometries(h, w):
        flow = torch.randn(2, 2, *geom.size, generator=g) * 30
        for kind, pred in (('flow', flow), ('disparity', flow[:, 0].abs().contiguous()), ('depth', flow[:, 1:].abs().contiguous() + 0.1)):
            plain = geom.restore(pred, kind)
            got = geom.restore(pred, kind, hflip=True)
            assert got.shape == plain.shape and got.is_contiguous() and torch.equal(got, torch.flip(plain, [-1])), (geom, kind)
            both = torch.full((4,) + tuple(plain.shape[1:]), -7.0)
            back = geom.restore(pred, kind, hflip=True, out=both[2:])
            assert back.data_ptr() == both[2:].data_ptr() and torch.equal(both[2:], got) and (both[:2] == -7.0).all()
            geom.restore(pred, kind, out=both[:2])
            assert torch.equal(both[:2], plain)
        with pytest.raises(ValueError):
            geom.restore(flow, 'flow', out=torch.zeros(1, 2, h, w))


# ------------------------------------------------------------------ 2. predict: the stereo views through the injected oracle
def build(name, h, w, batch=1):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    i0, i1 = synth_images(batch, h, w, seed=1000, kind='shift', normalized=(fk['task'] != 'flow'))
    kw = dict(fk)
    if fk['task'] == 'depth':
        k, pose = synth_camera(batch, h, w)
        kw.update(intrinsics=k, pose=pose)
    return model.bind_ops(OracleOps()), i0, i1, kw


def manual_views(model, geom, left, right, kw, right_disp, bidir, normalize=False):
    """evaluate_stereo.py:790-841 written out with torch.flip / torch.cat around ``model(...)``, the restore included."""
    a, b = geom.prepare(left, right, normalize=normalize)
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


@pytest.mark.parametrize('batch,h,w,size', [(2, 64, 96, None), (1, 37, 53, (64, 64)), (1, 59, 90, None)])
@pytest.mark.parametrize('right_disp,bidir', [(True, False), (False, True), (True, True)])
def test_predict_stereo_views_equal_the_manual_composition(batch, h, w, size, right_disp, bidir):
    model, left, right, kw = build('gmstereo_s1', h, w, batch)
    geom = prepost.geometry_for((h, w), size, 32, 'sintel')
    want = manual_views(model, geom, left, right, kw, right_disp, bidir)
    out = model.predict(left, right, inference_size=size, pred_right_disp=right_disp, pred_bidir_disp=bidir, **kw)
    got = out['flow_preds'][-1]
    assert list(out) == ['flow_preds'] and got.shape == ((2 if bidir else 1) * batch, h, w)
    assert torch.equal(got, want)
    plain = model.predict(left, right, inference_size=size, **kw)['flow_preds'][-1]
    if bidir:                                                   # one half is the ordinary prediction of the pair (samples are independent)
        ordinary, views = (got[batch:], got[:batch]) if right_disp else (got[:batch], got[batch:])
        assert (ordinary - plain).abs().max() <= 1e-4 * plain.abs().max()
        assert not torch.equal(views, plain)
    else:
        assert not torch.equal(got, plain)


def test_predict_stereo_views_take_uint8_frames_and_refuse_other_tasks():
    model, _, _, kw = build('gmstereo_s1', 37, 53)
    left, right = frames(1, 37, 53, seed=1), frames(1, 37, 53, seed=2)
    geom = prepost.geometry_for((37, 53), (64, 64), 32, 'sintel')
    for right_disp, bidir in ((True, False), (False, True)):
        want = manual_views(model, geom, left, right, kw, right_disp, bidir, normalize=True)
        got = model.predict(left, right, inference_size=(64, 64), pred_right_disp=right_disp, pred_bidir_disp=bidir, **kw)
        assert torch.equal(got['flow_preds'][-1], want)
    flow, i0, i1, fkw = build('gmflow_s1', 59, 90)
    for views in (dict(pred_right_disp=True), dict(pred_bidir_disp=True)):
        with pytest.raises(ValueError):
            flow.predict(i0, i1, **views, **fkw)
    depth, i0, i1, dkw = build('gmdepth_s1', 48, 64)
    with pytest.raises(ValueError):
        depth.predict(i0, i1, pred_bidir_disp=True, **dkw)
    # off by default and not passed on: the ordinary call is what it was
    assert torch.equal(model.predict(left, right, pred_right_disp=False, pred_bidir_disp=False, **kw)['flow_preds'][-1],
                       model.predict(left, right, **kw)['flow_preds'][-1])


# ------------------------------------------------------------------ 3. the runners, with a stand-in model
class StandIn:
    """Stands in for the model in the runners: ``predict`` resizes through the real geometry and "predicts" a smooth function of
    the prepared images (for the stereo views: of the views the real ``predict`` would hand the model)."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _value(a, b):
        return (a[:, 0] - 0.5 * b[:, 1]).abs() + 0.05 * a[:, 2].abs() + 0.5

    def predict(self, img0, img1, inference_size=None, pred_right_disp=False, pred_bidir_disp=False, task='flow', **kw):
        self.calls.append(dict(kw, task=task, inference_size=inference_size, shape=tuple(img0.shape)))
        geom = InferenceGeometry.resized(prepost.image_size(img0), inference_size)
        a, b = geom.prepare(img0, img1, normalize=True)
        if task == 'depth':
            pred = self._value(a, b)
            if kw.get('pred_bidir_depth'):
                pred = torch.cat((pred, self._value(b, a)), 0)
            return {'flow_preds': [geom.restore(pred, 'depth')]}
        fa, fb = torch.flip(a, [-1]), torch.flip(b, [-1])
        if pred_bidir_disp:
            pred = torch.cat((self._value(a, b), torch.flip(self._value(fb, fa), [-1])), 0)
        elif pred_right_disp:
            pred = torch.flip(self._value(fb, fa), [-1])
        else:
            pred = self._value(a, b)
        return {'flow_preds': [geom.restore(pred.contiguous(), 'disparity')]}


def write_frames(directory, names, h, w, seed):
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = []
    for name in names:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        io.write_png8(os.path.join(directory, name), img)
        out.append(img)
    return out


def read_png(path):
    from PIL import Image
    return np.array(Image.open(path))


@pytest.mark.parametrize('layout', ['dir', 'left-right'])
@pytest.mark.parametrize('bidir,batch_size', [(False, 1), (True, 2)])
def test_run_stereo_writes_the_reference_file_set(tmp_path, layout, bidir, batch_size):
    pytest.importorskip('PIL')
    from unimatch_amd import stereo
    h, w = 20, 30
    if layout == 'dir':
        names = [f'{i:02d}_{side}.png' for i in range(3) for side in ('a', 'b')]              # sorted: left, right alternate
        write_frames(str(tmp_path / 'in'), names, h, w, seed=3)
        lefts, rights = stereo.pair_lists(str(tmp_path / 'in'))
    else:
        write_frames(str(tmp_path / 'l'), [f'{i:02d}.png' for i in range(3)], h, w, seed=4)
        write_frames(str(tmp_path / 'r'), [f'{i:02d}.png' for i in range(3)], h, w, seed=5)
        lefts, rights = stereo.pair_lists(None, str(tmp_path / 'l'), str(tmp_path / 'r'))
    assert len(lefts) == len(rights) == 3
    model = StandIn()
    out = tmp_path / 'out'
    n = stereo.run_stereo(model, lefts, rights, str(out), {'attn_type': 'x', 'task': 'stereo'}, padding_factor=16,
                          pred_bidir_disp=bidir, save_pfm_disp=True, batch_size=batch_size, device='cpu')
    assert n == 3
    stems = [os.path.splitext(os.path.basename(p))[0] for p in lefts]
    suffixes = ['_disp'] + (['_disp_right'] if bidir else [])
    assert sorted(os.listdir(out)) == sorted(s + x + e for s in stems for x in suffixes for e in ('.png', '.pfm'))
    assert all(c['inference_size'] == (32, 32) and c['task'] == 'stereo' and c['attn_type'] == 'x' for c in model.calls)
    assert [c['shape'][0] for c in model.calls] == ([1, 1, 1] if batch_size == 1 else [2, 1])
    from unimatch_amd.video import read_frame_u8
    for i, stem in enumerate(stems):
        left, right = read_frame_u8(lefts[i])[None], read_frame_u8(rights[i])[None]
        want = StandIn().predict(left, right, inference_size=(32, 32), pred_bidir_disp=bidir, task='stereo')['flow_preds'][-1]
        for j, suffix in enumerate(suffixes):
            pfm, scale = io.read_pfm(str(out / (stem + suffix + '.pfm')))
            assert scale == 1 and pfm.shape == (h, w) and np.array_equal(pfm, want[j].numpy())
            png = read_png(str(out / (stem + suffix + '.png')))
            assert np.array_equal(png, visualize.disparity_to_image(want[j:j + 1])[0].numpy())
    with pytest.raises(ValueError):
        stereo.run_stereo(model, lefts, rights[:2], str(out), {}, device='cpu')
    with pytest.raises(ValueError):
        stereo.pair_lists(None, str(tmp_path), None)


def test_run_stereo_right_disp_and_inference_size(tmp_path):
    pytest.importorskip('PIL')
    from unimatch_amd import stereo
    from unimatch_amd.video import read_frame_u8
    write_frames(str(tmp_path / 'in'), ['a.png', 'b.png'], 20, 30, seed=6)
    lefts, rights = stereo.pair_lists(str(tmp_path / 'in'))
    n = stereo.run_stereo(StandIn(), lefts, rights, str(tmp_path / 'out'), {}, inference_size=(16, 48), pred_right_disp=True, device='cpu')
    assert n == 1 and os.listdir(tmp_path / 'out') == ['a_disp.png']
    want = StandIn().predict(read_frame_u8(lefts[0])[None], read_frame_u8(rights[0])[None], inference_size=(16, 48),
                             pred_right_disp=True, task='stereo')['flow_preds'][-1]
    assert np.array_equal(read_png(str(tmp_path / 'out' / 'a_disp.png')), visualize.disparity_to_image(want)[0].numpy())


@pytest.mark.parametrize('bidir', [False, True])
def test_run_depth_reads_a_scannet_scene_and_writes_the_reference_file_set(tmp_path, bidir):
    pytest.importorskip('PIL')
    from unimatch_amd import depth
    from unimatch_amd.video import read_frame_u8
    h, w = 24, 40
    scene = tmp_path / 'scene'
    names = [f'{i:04d}.png' for i in (0, 20, 40)]
    write_frames(str(scene / 'color'), names, h, w, seed=8)
    (scene / 'pose').mkdir()
    (scene / 'intrinsic').mkdir()
    rng = np.random.default_rng(9)
    poses = []
    for i, name in enumerate(names):
        ang = 0.03 * i
        p = np.eye(4)
        p[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        p[:3, 3] = rng.standard_normal(3) * 0.1
        poses.append(p)
        np.savetxt(str(scene / 'pose' / name.replace('.png', '.txt')), p, delimiter=' ')
    k4 = np.eye(4)
    k4[:3, :3] = [[577.59, 0, 20.1], [0, 578.73, 12.2], [0, 0, 1]]
    np.savetxt(str(scene / 'intrinsic' / 'intrinsic_depth.txt'), k4)
    imgs, p, k = depth.read_scene(str(scene))
    assert len(imgs) == 3 and p.shape == (3, 4, 4) and p.dtype == k.dtype == np.float32
    assert np.array_equal(k, k4[:3, :3].astype(np.float32))
    model = StandIn()
    out = tmp_path / 'out'
    n = depth.run_depth(model, str(scene), str(out), {'attn_type': 'swin', 'task': 'depth', 'min_depth': 0.1, 'max_depth': 2.0},
                        padding_factor=16, min_depth=0.5, max_depth=10., num_depth_candidates=32, pred_bidir_depth=bidir, device='cpu')
    assert n == 2
    assert sorted(os.listdir(out)) == sorted([s + e for s in ('0000', '0020') for e in (['.png', '_bwd.png'] if bidir else ['.png'])])
    for i, call in enumerate(model.calls):
        assert call['task'] == 'depth' and call['inference_size'] == (32, 48) and call['attn_type'] == 'swin'
        assert call['min_depth'] == 1 / 10. and call['max_depth'] == 1 / 0.5 and call['num_depth_candidates'] == 32
        assert call['pred_bidir_depth'] == bidir and call['depth_from_argmax'] is False
        assert torch.equal(call['intrinsics'], torch.from_numpy(k)[None])                       # not rescaled, as in the reference
        rel = np.linalg.inv(poses[i + 1].astype(np.float32)) @ poses[i].astype(np.float32)
        assert call['pose'].dtype == torch.float32 and np.array_equal(call['pose'][0].numpy(), rel.astype(np.float32))
    for i, stem in enumerate(('0000', '0020')):
        ref, tgt = read_frame_u8(imgs[i])[None], read_frame_u8(imgs[i + 1])[None]
        want = StandIn().predict(ref, tgt, inference_size=(32, 48), task='depth', pred_bidir_depth=bidir)['flow_preds'][-1]
        assert np.array_equal(read_png(str(out / (stem + '.png'))), visualize.inverse_depth_to_image(want[:1])[0].numpy())
        if bidir:
            assert np.array_equal(read_png(str(out / (stem + '_bwd.png'))), visualize.inverse_depth_to_image(want[1:])[0].numpy())
    # opt-in intrinsics scaling
    model = StandIn()
    depth.run_depth(model, str(scene), str(out), {}, padding_factor=16, scale_intrinsics=True, device='cpu')
    want_k = InferenceGeometry.resized((h, w), (32, 48)).scaled_intrinsics(torch.from_numpy(k)[None])
    assert torch.equal(model.calls[0]['intrinsics'], want_k) and not torch.equal(want_k, torch.from_numpy(k)[None])
    with pytest.raises(FileNotFoundError):
        depth.read_scene(str(tmp_path / 'nowhere'))


def test_parsers_offer_the_task_configurations():
    from unimatch_amd import depth, stereo
    with pytest.raises(SystemExit):
        stereo.main(['--dir', 'x', '--out', 'y', '--model-config', 'gmflow_s1'])
    with pytest.raises(SystemExit):
        depth.main(['--scene', 'x', '--out', 'y', '--model-config', 'gmstereo_s1'])
