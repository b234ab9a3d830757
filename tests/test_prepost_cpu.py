"""CPU tests of the inference-size handling (unimatch_amd/prepost.py): the host restatement of the two kernels against
``F.interpolate`` and ``io.InputPadder``, the rescale / transpose rules against written-out copies of the reference's lines, the
argument checks of the C ABI, ``UniMatch.predict`` with the oracle injected as backend, and the stereo / depth validation loops on a
model that replays recorded predictions.

Bound of the resize comparisons: ``4 * 2^-23 * max|input|``.  Both sides evaluate the same convex combination with the same fp32
weights; they differ only in the order of at most seven fp32 operations, each of which contributes at most half an ulp of a value
that is bounded by ``max|input|``."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unimatch_amd import UniMatch, _abi, evaluate, io, metrics, prepost
from unimatch_amd.prepost import InferenceGeometry
from unimatch_amd.synth import CONFIGS, synth_camera, synth_images, synth_state_dict
from tests.metrics_util import check_result, load_golden
from tests.oracle_ops import OracleOps

ULP4 = 4 * 2.0 ** -23
RESIZES = [((436, 1024), (448, 1024)), ((1080, 1920), (768, 1344)), ((375, 1242), (384, 1248)), ((480, 640), (448, 576)),
           ((768, 1344), (1080, 1920)), ((77, 131), (64, 96)), ((77, 131), (1, 96)), ((40, 1), (64, 8)), ((64, 96), (64, 96))]


def images(b, h, w, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    return x if u8 else x.permute(0, 3, 1, 2).float().contiguous()


# ------------------------------------------------------------------ 1. the restatement's resize against F.interpolate
@pytest.mark.parametrize('src,dst', RESIZES)
def test_host_resize_against_interpolate(src, dst):
    x = images(1, *src, seed=src[0] + dst[1])
    x[0, 0, 0, 0], x[0, 1, -1, -1] = 255.0, 255.0
    got = prepost.resize_host(x, dst)
    want = F.interpolate(x, size=dst, mode='bilinear', align_corners=True)
    err = (got - want).abs().max().item()
    bound = ULP4 * x.abs().max().item()
    print(f'{src} -> {dst}: max |restatement - F.interpolate| = {err:.3g} (bound {bound:.3g})')
    assert got.shape == want.shape and got.dtype == torch.float32
    assert err <= bound
    if src == dst:
        assert torch.equal(got, x)
    # through the geometry object, and for a prediction (no rescale for depth)
    geom = InferenceGeometry.resized((1, 3) + src, dst)
    assert torch.equal(geom.prepare(x)[0], got if src != dst else x)
    back = InferenceGeometry.resized((1, 3) + dst, src).restore(x[:, 0], 'depth')
    assert torch.equal(back, got[:, 0] if src != dst else x[:, 0])


# ------------------------------------------------------------------ 2. padding is InputPadder's, bit for bit
@pytest.mark.parametrize('mode', ['sintel', 'kitti'])
@pytest.mark.parametrize('h,w,factor', [(436, 1024, 8), (375, 1242, 32), (37, 53, 16), (64, 96, 32), (125, 189, 8), (1, 1, 8)])
def test_padded_is_the_input_padder(mode, h, w, factor):
    x, y = images(2, h, w, seed=h), images(2, h, w, seed=w + 1)
    padder = io.InputPadder(x.shape, mode=mode, padding_factor=factor)
    geom = InferenceGeometry.padded(x.shape, mode, factor)
    want = padder.pad(x, y)
    got = geom.prepare(x, y)
    assert geom._pad == padder._pad and geom.crop == (padder._pad[2], padder._pad[0])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    pred = torch.randn(2, 2, *geom.size, generator=torch.Generator().manual_seed(3))
    assert torch.equal(geom.restore(pred, 'flow'), padder.unpad(pred))
    assert torch.equal(geom.restore(pred[:, 0], 'disparity'), padder.unpad(pred[:, 0]))
    assert torch.equal(geom.restore(geom.prepare(x)[0][:, :2], 'flow'), x[:, :2])         # restore(prepare(x)) is x
    if (h % factor, w % factor) == (0, 0):
        assert geom.identity and got[0] is x and geom.restore(pred, 'flow') is pred      # nothing to do: the input itself
    # uint8 frames: the same values
    u = images(2, h, w, seed=h, u8=True)
    assert torch.equal(geom.prepare(u)[0], want[0])


# ------------------------------------------------------------------ 3. rescaling and transposition: the reference's lines
def reference_flow_block(image1, image2, inference_size, model):
    """evaluate_flow.py:713-758, written out."""
    transpose_img = False
    if image1.size(-2) > image1.size(-1):
        image1 = torch.transpose(image1, -2, -1)
        image2 = torch.transpose(image2, -2, -1)
        transpose_img = True
    ori_size = image1.shape[-2:]
    if inference_size[0] != ori_size[0] or inference_size[1] != ori_size[1]:
        image1 = F.interpolate(image1, size=inference_size, mode='bilinear', align_corners=True)
        image2 = F.interpolate(image2, size=inference_size, mode='bilinear', align_corners=True)
    flow_pr = model(image1, image2)
    if inference_size[0] != ori_size[0] or inference_size[1] != ori_size[1]:
        flow_pr = F.interpolate(flow_pr, size=ori_size, mode='bilinear', align_corners=True)
        flow_pr[:, 0] = flow_pr[:, 0] * ori_size[-1] / inference_size[-1]
        flow_pr[:, 1] = flow_pr[:, 1] * ori_size[-2] / inference_size[-2]
    if transpose_img:
        flow_pr = torch.transpose(flow_pr, -2, -1)
    return flow_pr


@pytest.mark.parametrize('h,w,size', [(100, 60, (64, 96)), (60, 100, (64, 96)), (375, 1242, (384, 1248)), (97, 64, (64, 104)),
                                      (96, 64, (64, 96))])
def test_flow_scale_and_unswapped_channels_under_transpose(h, w, size):
    x, y = images(2, h, w, seed=7), images(2, h, w, seed=8)
    seen = {}

    def model(a, b):                                   # a "flow" that depends on the position and on the channel
        seen['in'] = (a, b)
        gy, gx = torch.meshgrid(torch.arange(a.shape[-2]).float(), torch.arange(a.shape[-1]).float(), indexing='ij')
        return torch.stack([gx * 0.37 + a[:, 0] * 0.01, -gy * 0.91 + b[:, 1] * 0.01], 1)

    want = reference_flow_block(x, y, size, model)
    ref_in = seen['in']
    geom = InferenceGeometry.resized(x.shape, size, transpose='auto')
    assert geom.transpose == (h > w) and geom.shape == (h, w)
    a, b = geom.prepare(x, y)
    bound = ULP4 * 255.0
    assert (a - ref_in[0]).abs().max() <= bound and (b - ref_in[1]).abs().max() <= bound
    got = geom.restore(model(*ref_in), 'flow')         # the same prediction on both sides: only the restore differs
    assert got.shape == want.shape == (2, 2, h, w)
    peak = model(*ref_in).abs().max().item() * max(geom.image_size[1] / size[1], geom.image_size[0] / size[0], 1.0)
    assert (got - want).abs().max().item() <= ULP4 * peak
    # the scale factors themselves, on a constant prediction: u * W / wp and v * H / hp of the TRANSPOSED frame, channels in place
    ones = torch.ones(1, 2, *size)
    ih, iw = geom.image_size
    r = geom.restore(ones, 'flow')
    if geom.mode == 'resize':
        assert r[0, 0].unique().tolist() == [(torch.tensor(1.0) * iw / size[1]).item()]
        assert r[0, 1].unique().tolist() == [(torch.tensor(1.0) * ih / size[0]).item()]
    else:
        assert torch.equal(r, ones.transpose(-2, -1) if geom.transpose else ones)


def test_disparity_scale_and_no_scale_for_depth():
    h, w, size = 375, 1242, (384, 1280)
    pred = torch.rand(2, *size, generator=torch.Generator().manual_seed(5)) * 190
    geom = InferenceGeometry.resized((h, w), size)
    back = F.interpolate(pred.unsqueeze(1), size=(h, w), mode='bilinear', align_corners=True).squeeze(1)
    want_disp = back * w / float(size[-1])                                   # evaluate_stereo.py:373-375
    got = geom.restore(pred, 'disparity')
    assert got.shape == (2, h, w) and (got - want_disp).abs().max().item() <= ULP4 * 190 * w / size[1]
    mine = prepost.resize_host(pred.unsqueeze(1), (h, w)).squeeze(1)
    assert torch.equal(got, mine * w / float(size[-1]))                      # a multiply, then a divide
    depth = geom.restore(pred, 'depth')                                      # evaluate_depth.py:128-131: not rescaled
    assert torch.equal(depth, mine) and (depth - back).abs().max().item() <= ULP4 * 190
    with pytest.raises(ValueError):
        geom.restore(pred, 'flow')
    with pytest.raises(ValueError):
        geom.restore(pred, 'disp')


def test_constructors_and_intrinsics():
    g = InferenceGeometry.nearest((1, 3, 1080, 1920), 32)
    assert g.size == (1088, 1920) and g.mode == 'resize' and not g.transpose
    g = InferenceGeometry.nearest((1920, 1080), 32)                           # tall: transposed first (evaluate_flow.py:713-723)
    assert g.transpose and g.image_size == (1080, 1920) and g.size == (1088, 1920) and g.shape == (1920, 1080)
    assert InferenceGeometry.nearest((64, 96), 32).identity
    assert not InferenceGeometry.nearest((96, 64), 32).identity               # the transpose is still to do
    assert InferenceGeometry.padded((96, 64), 'kitti', 32, transpose='auto').size == (64, 96)
    with pytest.raises(ValueError):
        InferenceGeometry((64, 96), (32, 96), 'pad')
    with pytest.raises(ValueError):
        InferenceGeometry.resized((64, 96), (64, 0))
    with pytest.raises(ValueError):
        InferenceGeometry.resized((64, 96), (64, 128), transpose='yes')
    with pytest.raises(ValueError):
        InferenceGeometry.resized((64, 96), (64, 128)).prepare(torch.zeros(1, 3, 64, 97))
    k = torch.tensor([[500.0, 0, 320], [0, 510.0, 240], [0, 0, 1]])
    g = InferenceGeometry.resized((480, 640), (448, 576))
    s = g.scaled_intrinsics(k[None])
    assert torch.allclose(s[0, 0], k[0] * (575 / 639)) and torch.allclose(s[0, 1], k[1] * (447 / 479)) and torch.equal(s[0, 2], k[2])
    with pytest.raises(ValueError):
        InferenceGeometry.padded((37, 53), 'sintel', 8).scaled_intrinsics(k)


# ------------------------------------------------------------------ 4. normalisation
@pytest.mark.parametrize('layout', ['u8', 'f32'])
def test_normalisation_is_the_loaders_expression(layout):
    u = images(2, 37, 53, seed=11, u8=True)
    u[0, :16, :16] = torch.arange(256, dtype=torch.uint8).view(16, 16, 1)                # every grey level
    x = u if layout == 'u8' else u.permute(0, 3, 1, 2).float().contiguous()
    mean = torch.tensor(prepost.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(prepost.IMAGENET_STD).view(1, 3, 1, 1)
    want = (u.permute(0, 3, 1, 2).float() / 255 - mean) / std
    # ... which is three separately rounded IEEE operations (NumPy float32)
    f = u.permute(0, 3, 1, 2).numpy().astype(np.float32)
    assert np.array_equal(want.numpy(), (f / np.float32(255) - mean.numpy()) / std.numpy())
    got = InferenceGeometry.padded((37, 53), 'kitti', 1).prepare(x, normalize=True)[0]
    assert torch.equal(got, want)
    geom = InferenceGeometry.padded((37, 53), 'kitti', 16)
    assert torch.equal(geom.prepare(x, normalize=True)[0], io.InputPadder((37, 53), 'kitti', 16).pad(want)[0])
    custom = ((0.5, 0.25, 0.125), (0.5, 2.0, 0.3))
    m, s = (torch.tensor(c).view(1, 3, 1, 1) for c in custom)
    assert torch.equal(geom.prepare(x, normalize=custom)[0], io.InputPadder((37, 53), 'kitti', 16).pad((f_t(u) / 255 - m) / s)[0])
    # normalise first, then resize: the blends see normalised values
    rg = InferenceGeometry.resized((37, 53), (32, 64))
    assert torch.equal(rg.prepare(x, normalize=True)[0], prepost.resize_host(want, (32, 64)))
    with pytest.raises(ValueError):
        geom.prepare(x, normalize=((0, 0, 0), (1, 0, 1)))


def f_t(u):
    return u.permute(0, 3, 1, 2).float()


# ------------------------------------------------------------------ 5. argument errors of the C ABI, without a GPU
def test_abi_argument_errors_without_gpu():
    lib = _abi.load()
    fake = ctypes.c_void_p(4096)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (ctypes.c_float * 3)(0.5, 0.0, 0.5)

    def prep(src=fake, layout=0, dst=fake, b=1, h=37, w=53, tr=0, mean=None, std=None, mode=0, hp=40, wp=56, top=1, left=1):
        return lib.um_image_prepare(src, layout, dst, b, h, w, tr, mean, std, mode, hp, wp, top, left, None)

    assert prep(src=None) == -1 and b'um_image_prepare' in lib.um_last_error_string()
    assert prep(dst=None) == -1
    assert prep(layout=2) == -1
    assert prep(b=0) == -1 and prep(h=0) == -1 and prep(hp=0) == -1 and prep(b=30000) == -1
    assert prep(mode=2) == -1
    assert prep(h=262141, hp=262144, wp=56, w=53) == -1 and prep(mode=1, hp=262141) == -1       # rows beyond the grid's reach
    assert prep(top=4) == -1 and prep(left=-1) == -1 and prep(hp=36) == -1          # the image leaves the padded frame
    assert prep(tr=1) == -1                                                          # transposed: 53 x 37 does not fit 40 x 56
    assert prep(mean=f3) == -1 and prep(std=f3) == -1                                # mean and std come together
    assert prep(mean=f3, std=z3) == -1                                               # a zero std

    def rest(pred=fake, out=fake, b=1, c=2, hp=40, wp=56, mode=0, top=1, left=1, h=37, w=53, kind=0, tr=0):
        return lib.um_pred_restore(pred, out, b, c, hp, wp, mode, top, left, h, w, kind, tr, None)

    assert rest(pred=None) == -1 and b'um_pred_restore' in lib.um_last_error_string()
    assert rest(out=None) == -1
    assert rest(c=1) == -1 and rest(c=2, kind=1) == -1 and rest(c=2, kind=2) == -1 and rest(c=1, kind=3) == -1
    assert rest(b=0) == -1 and rest(w=0) == -1 and rest(b=40000) == -1
    assert rest(mode=-1) == -1
    assert rest(mode=1, h=262141) == -1 and rest(mode=1, hp=262141) == -1 and rest(mode=1, c=1, kind=2, w=262141) == -1
    assert rest(top=4) == -1 and rest(left=4) == -1 and rest(tr=1) == -1
    # the Python wrappers refuse host tensors and bad modes before anything is loaded onto a GPU
    from unimatch_amd.ops import HipOps
    ops = HipOps.__new__(HipOps)
    with pytest.raises(ValueError):
        HipOps.image_prepare(ops, torch.zeros(1, 3, 8, 8), (8, 8))
    with pytest.raises(ValueError):
        HipOps.pred_restore(ops, torch.zeros(1, 2, 8, 8), (8, 8))
    with pytest.raises(ValueError):
        HipOps.pred_restore(ops, torch.zeros(1, 2, 8, 8), (8, 8), kind='disp')


# ------------------------------------------------------------------ 6. predict with the oracle injected
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


@pytest.mark.parametrize('name,h,w', [('gmflow_s1', 59, 90), ('gmstereo_s1', 59, 90), ('gmdepth_s1', 90, 120)])
def test_predict_padded_equals_pad_forward_unpad(name, h, w):
    model, i0, i1, kw = build(name, h, w)
    task = kw['task']
    factor, mode = {'flow': (8, 'sintel'), 'stereo': (32, 'sintel'), 'depth': (16, 'kitti')}[task]
    padder = io.InputPadder(i0.shape, mode=mode, padding_factor=factor)
    a, b = padder.pad(i0, i1)
    want = padder.unpad(model(a, b, **kw)['flow_preds'][-1])
    out = model.predict(i0, i1, **kw)
    assert list(out) == ['flow_preds'] and len(out['flow_preds']) == 1
    assert torch.equal(out['flow_preds'][-1], want) and want.shape[-2:] == (h, w)
    # an explicit factor / mode
    padder = io.InputPadder(i0.shape, mode='kitti', padding_factor=32)
    a, b = padder.pad(i0, i1)
    want = padder.unpad(model(a, b, **kw)['flow_preds'][-1])
    assert torch.equal(model.predict(i0, i1, padding_factor=32, pad_mode='kitti', **kw)['flow_preds'][-1], want)


@pytest.mark.parametrize('name,h,w,size', [('gmflow_s1', 59, 90, (64, 96)), ('gmflow_s1', 90, 59, (64, 96)),
                                           ('gmstereo_s1', 59, 90, (64, 96)), ('gmdepth_s1', 90, 120, (96, 128))])
def test_predict_resized_equals_resize_forward_resize_back(name, h, w, size):
    model, i0, i1, kw = build(name, h, w)
    task = kw['task']
    # the model sees what the restatement prepared (the restatement against F.interpolate is test 1), so that what remains is the
    # reference's resize-back and rescale of the SAME prediction
    geom = InferenceGeometry.resized(i0.shape, size, transpose=(task == 'flow' and h > w))
    a, b = geom.prepare(i0, i1)
    ih, iw = geom.image_size
    for x, y in ((a, i0), (b, i1)):
        y = y.transpose(-2, -1) if geom.transpose else y
        assert (x - F.interpolate(y, size=size, mode='bilinear', align_corners=True)).abs().max() <= ULP4 * y.abs().max()
    pred = model(a, b, **kw)['flow_preds'][-1]
    if task == 'flow':
        want = F.interpolate(pred, size=(ih, iw), mode='bilinear', align_corners=True)
        want[:, 0] = want[:, 0] * iw / size[-1]
        want[:, 1] = want[:, 1] * ih / size[-2]
        if geom.transpose:
            want = torch.transpose(want, -2, -1)
    else:
        want = F.interpolate(pred.unsqueeze(1), size=(ih, iw), mode='bilinear', align_corners=True).squeeze(1)
        if task == 'stereo':
            want = want * iw / float(size[-1])
    got = model.predict(i0, i1, inference_size=size, **kw)['flow_preds'][-1]
    factor = max(iw / size[1], ih / size[0], 1.0) if task != 'depth' else 1.0
    err, bound = (got - want).abs().max().item(), ULP4 * pred.abs().max().item() * factor
    print(f'{name} {h}x{w} -> {size}: max |predict - torch ops| = {err:.3g} (bound {bound:.3g})')
    assert got.shape == want.shape and got.shape[-2:] == (h, w) and err <= bound


@pytest.mark.parametrize('name,h,w,size', [('gmflow_s1', 127, 191, (64, 96)), ('gmflow_s1', 191, 127, (64, 96)),
                                           ('gmstereo_s1', 127, 191, (64, 96)), ('gmdepth_s1', 191, 255, (96, 128))])
def test_predict_resized_equals_the_by_hand_torch_sequence(name, h, w, size):
    """``predict`` against nothing but torch ops: transpose, ``F.interpolate``, forward, ``F.interpolate`` back, the rescale lines.
    The sizes have ``(in - 1) = 2 (out - 1)``, so the forward resize picks every second pixel exactly on both sides and the model sees
    the same bits; with fractional weights its input would differ by a rounding, which the model amplifies (that case is the test
    above, where the prepared input is held to ``F.interpolate`` and shared)."""
    model, i0, i1, kw = build(name, h, w)
    task = kw['task']
    tr = task == 'flow' and h > w
    a, b = ((x.transpose(-2, -1) if tr else x) for x in (i0, i1))
    ori = tuple(a.shape[-2:])
    a, b = (F.interpolate(x, size=size, mode='bilinear', align_corners=True) for x in (a, b))
    pred = model(a, b, **kw)['flow_preds'][-1]
    if task == 'flow':
        want = F.interpolate(pred, size=ori, mode='bilinear', align_corners=True)
        want[:, 0] = want[:, 0] * ori[-1] / size[-1]
        want[:, 1] = want[:, 1] * ori[-2] / size[-2]
        want = torch.transpose(want, -2, -1) if tr else want
    else:
        want = F.interpolate(pred.unsqueeze(1), size=ori, mode='bilinear', align_corners=True).squeeze(1)
        want = want * ori[-1] / float(size[-1]) if task == 'stereo' else want
    got = model.predict(i0, i1, inference_size=size, **kw)['flow_preds'][-1]
    factor = max(ori[1] / size[1], ori[0] / size[0], 1.0) if task != 'depth' else 1.0
    err, bound = (got - want).abs().max().item(), ULP4 * pred.abs().max().item() * factor
    print(f'{name} {h}x{w} -> {size}: max |predict - by-hand torch sequence| = {err:.3g} (bound {bound:.3g})')
    assert got.shape == want.shape and got.shape[-2:] == (h, w) and err <= bound


def test_predict_takes_uint8_frames_and_normalises_by_task():
    model, i0, i1, kw = build('gmstereo_s1', 59, 90)
    g = torch.Generator().manual_seed(2)
    u0, u1 = (torch.randint(0, 256, (1, 59, 90, 3), generator=g, dtype=torch.uint8) for _ in range(2))
    mean, std = (torch.tensor(c).view(1, 3, 1, 1) for c in (prepost.IMAGENET_MEAN, prepost.IMAGENET_STD))
    n0, n1 = ((f_t(u) / 255 - mean) / std for u in (u0, u1))
    want = model.predict(n0, n1, **kw)['flow_preds'][-1]                         # fp32 input: already normalised, left alone
    assert torch.equal(model.predict(u0, u1, **kw)['flow_preds'][-1], want)
    assert not torch.equal(model.predict(u0, u1, normalize=False, **kw)['flow_preds'][-1], want)
    flow, _, _, fkw = build('gmflow_s1', 59, 90)
    want = flow.predict(f_t(u0), f_t(u1), **fkw)['flow_preds'][-1]               # flow: raw 0..255, the model normalises
    assert torch.equal(flow.predict(u0, u1, **fkw)['flow_preds'][-1], want)
    with pytest.raises(ValueError):
        flow.predict(u0, f_t(u1), **fkw)


# ------------------------------------------------------------------ 6b. the validation loops on a model that replays predictions
class Replay:
    """Stands in for the model: returns the next recorded prediction, brought to the size of the images it is given by ``place``."""

    def __init__(self, preds, place):
        self.preds, self.place, self.calls = list(preds), place, []

    def __call__(self, img0, img1, **kw):
        self.calls.append((tuple(img0.shape), kw))
        n = img0.shape[0]
        batch, self.preds = torch.stack(self.preds[:n], 0), self.preds[n:]
        return {'flow_preds': [self.place(batch, tuple(img0.shape[-2:]))]}


def test_validate_stereo_on_recorded_predictions():
    g = load_golden()
    n, h, w = g['disp_gt'].shape
    gt, pred = torch.from_numpy(g['disp_gt']), torch.from_numpy(g['disp_pred'])
    gt = torch.cat([gt, torch.zeros(1, h, w)], 0)                               # a sample without a valid pixel: skipped
    pred = torch.cat([pred, torch.ones(1, h, w)], 0)
    frames = [torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(i), dtype=torch.uint8) for i in range(n + 1)]
    samples = [(frames[i], frames[i], gt[i]) for i in range(n + 1)]
    padder = io.InputPadder((h, w), padding_factor=32)
    for tag, max_disp in (('all', 0.0), ('things', float(g['disp_max_disp']))):
        for batch_size in (1, 3):
            model = Replay(pred, lambda p, size: padder.pad(p)[0])
            res = evaluate.validate_stereo(model, samples, 'kitti15', padding_factor=32, max_disp=max_disp, batch_size=batch_size,
                                           attn_type='self_swin2d_cross_1d')
            assert set(res) == {'kitti15_epe', 'kitti15_d1', 'kitti15_3px'}
            assert all(c[0][-2:] == (64, 64) and c[1]['task'] == 'stereo' for c in model.calls)
            for key, name in (('epe', 'epe'), ('d1', 'd1'), ('3px', 'thres3')):    # the reference's mean of per-sample values
                check_result(name, res['kitti15_' + key], np.float32(np.mean(g[f'disp_{tag}/{name}'].astype(np.float64))), f'{tag} ')
    # the resize path: resize back, scale by W / wp (evaluate_stereo.py:373-375), then the same metrics
    size = (64, 96)
    up = lambda p, s: F.interpolate(p.unsqueeze(1), size=s, mode='bilinear', align_corners=True).squeeze(1) * 1.7
    res = evaluate.validate_stereo(Replay(pred, up), samples, 'things', inference_size=size, max_disp=150.0)
    want = metrics.StereoMetrics(150.0)
    for i in range(n + 1):
        back = F.interpolate(up(pred[i:i + 1], size).unsqueeze(1), size=(h, w), mode='bilinear', align_corners=True).squeeze(1)
        want.update(back * w / float(size[-1]), gt[i:i + 1])
    want = want.compute()
    assert want['skipped'] == 1
    for key, name in (('epe', 'epe'), ('d1', 'd1'), ('3px', 'thres3')):
        assert abs(res['things_' + key] - want[name]) <= 2e-6 * abs(want[name]), (key, res, want)


def test_validate_depth_on_recorded_predictions():
    g = load_golden()
    n, h, w = g['depth_gt'].shape
    lo, hi = (float(v) for v in g['depth_range'])
    gt, pred, valid = (torch.from_numpy(g[k]) for k in ('depth_gt', 'depth_pred', 'depth_valid'))
    gt, pred, valid = torch.cat([gt, gt[:1]], 0), torch.cat([pred, pred[:1]], 0), torch.cat([valid, torch.zeros(1, h, w)], 0)
    k, pose = synth_camera(1, h, w)
    img = torch.zeros(3, h, w)
    samples = [(img, img, k[0], pose[0], gt[i], valid[i]) for i in range(n + 1)]
    padder = io.InputPadder((h, w), mode='kitti', padding_factor=16)
    model = Replay(pred, lambda p, size: padder.pad(p)[0])
    res = evaluate.validate_depth(model, samples, 'scannet', padding_factor=16, min_depth=lo, max_depth=hi, attn_type='swin')
    assert set(res) == {'scannet_' + e for e in evaluate.DEPTH_ERRORS}
    shape, kw = model.calls[0]
    assert shape[-2:] == (48, 64) and kw['task'] == 'depth' and kw['min_depth'] == 1 / hi and kw['max_depth'] == 1 / lo
    assert tuple(kw['intrinsics'].shape) == (1, 3, 3) and tuple(kw['pose'].shape) == (1, 4, 4)
    for name in evaluate.DEPTH_ERRORS:                                          # the sample with an empty mask does not count
        rec = g[f'depth/{name}']
        check_result(name, res['scannet_' + name], np.mean(rec.astype(np.float64)).astype(rec.dtype), 'depth ')
    # resized: the prediction is resized back and NOT rescaled (evaluate_depth.py:128-131); bare names for an empty prefix
    size = (48, 80)
    up = lambda p, s: F.interpolate(p.unsqueeze(1), size=s, mode='bilinear', align_corners=True).squeeze(1)
    res = evaluate.validate_depth(Replay(pred, up), samples, '', inference_size=size, min_depth=lo, max_depth=hi)
    want = metrics.DepthMetrics(lo, hi)
    for i in range(n + 1):
        back = F.interpolate(up(pred[i:i + 1], size).unsqueeze(1), size=(h, w), mode='bilinear', align_corners=True).squeeze(1)
        want.update(back, gt[i:i + 1], valid[i:i + 1])
    want = want.compute()
    assert set(res) == set(evaluate.DEPTH_ERRORS) and want['skipped'] == 1
    for name in evaluate.DEPTH_ERRORS:
        assert abs(res[name] - want[name]) <= 2e-6 * abs(want[name]), (name, res, want)


def test_kitti15_stereo_reader_and_parser(tmp_path):
    pytest.importorskip('PIL')
    from PIL import Image
    base = tmp_path / 'training'
    rng = np.random.default_rng(0)
    disp = (rng.random((20, 30)) * 90).astype(np.float32)
    for sub in ('image_2', 'image_3', 'disp_occ_0'):
        (base / sub).mkdir(parents=True)
    for i in range(2):
        for sub in ('image_2', 'image_3'):
            Image.fromarray(rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)).save(base / sub / f'{i:06d}_10.png')
        io.write_kitti_disp(str(base / 'disp_occ_0' / f'{i:06d}_10.png'), disp)
    pairs = evaluate.Kitti15StereoPairs(str(tmp_path))
    left, right, gt = pairs[1]
    assert len(pairs) == 2 and left.dtype == torch.uint8 and tuple(left.shape) == (20, 30, 3) and tuple(right.shape) == (20, 30, 3)
    assert gt.dtype == torch.float32 and torch.equal(gt, torch.from_numpy(np.floor(disp * 256) / 256).float())
    args = evaluate.build_parser().parse_args(['--dataset', 'kitti15-stereo', '--root', 'x', '--model-config', 'gmstereo_s1',
                                               '--padding-factor', '32', '--inference-size', '384', '1248'])
    assert args.dataset == 'kitti15-stereo' and args.inference_size == [384, 1248] and args.padding_factor == 32
    with pytest.raises(FileNotFoundError):
        evaluate.Kitti15StereoPairs(str(tmp_path / 'nowhere'))


# ------------------------------------------------------------------ the frame-directory driver with device_resize
class DifferenceModel:
    """Stands in for the model in ``video.run_directory``: the "flow" of a pair is the difference of two channels of its frames."""

    def forward_sequence(self, frames, pred_bidir_flow=False, pairs_per_launch=8, carry=None, **kw):
        seq = frames if carry is None else torch.cat([carry, frames], 0)
        out = {'flow': (seq[1:, :2] - seq[:-1, :2]).contiguous(), 'carry': seq[-1:]}
        if pred_bidir_flow:
            out['flow_bwd'] = -out['flow']
        return out


@pytest.mark.parametrize('h,w,inference_size', [(50, 76, None), (76, 50, None), (50, 76, (64, 96)), (48, 80, None)])
def test_run_directory_device_resize_writes_the_same_files(tmp_path, h, w, inference_size):
    pytest.importorskip('PIL')
    import os
    from unimatch_amd import video
    rng = np.random.default_rng(h)
    (tmp_path / 'in').mkdir()
    for i in range(6):
        io.write_png8(str(tmp_path / 'in' / f'{i:02d}.png'), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    paths = video.list_frames(str(tmp_path / 'in'))
    outs = []
    for flag in (False, True):
        out = tmp_path / f'out{int(flag)}'
        n = video.run_directory(DifferenceModel(), paths, str(out), {}, padding_factor=32, inference_size=inference_size,
                                pred_bidir_flow=True, save_flo=True, pairs_per_launch=2, device='cpu', device_resize=flag)
        assert n == 5
        outs.append(out)
    names = sorted(os.listdir(outs[0]))
    assert names == sorted(os.listdir(outs[1])) and len(names) == 5 * 4
    for name in (n for n in names if n.endswith('.flo')):
        a, b = io.read_flo(str(outs[0] / name)), io.read_flo(str(outs[1] / name))
        assert a.shape == b.shape == (h, w, 2)
        # a difference of two resized frames (each within 4 ulp of 255), resized back and scaled
        assert np.abs(a - b).max() <= 4 * ULP4 * 255 * 2
