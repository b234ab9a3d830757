"""CPU tests of the evaluation metrics: the host restatements against results recorded from the reference
(tests/golden/metrics.npz, minted by tests/golden/make_golden_metrics.py), batching and crop independence, ``validate_flow`` with a
stub model, the dataset readers, the command line, and the C ABI of the three kernels without a GPU.  The comparison rules are stated
in tests/metrics_util.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, evaluate, io, metrics
from tests.metrics_util import (REL_FLOAT64, SHARE_KEYS, check_result, check_share, check_sum, flow_pixels, load_golden, seeded_flow_case)

N, H, W = 4, 37, 53


@pytest.fixture(scope='module')
def golden():
    return load_golden()


def t(a):
    return torch.from_numpy(np.asarray(a))


def sintel_padder():
    return io.InputPadder((1, 3, H, W), mode='sintel', padding_factor=8)


def kitti_padder():
    return io.InputPadder((1, 3, H, W), mode='kitti', padding_factor=8)


def mean64(values):
    return float(np.mean(np.concatenate([np.ravel(v) for v in values]).astype(np.float64)))


# ------------------------------------------------------------------ flow
@pytest.mark.parametrize('dstype', ['clean', 'final'])
def test_sintel_results_match_the_reference(golden, dstype):
    pred, gt, noc = golden[f'sintel_{dstype}_pred'], golden[f'sintel_{dstype}_gt'], golden[f'sintel_{dstype}_noc']
    padder = sintel_padder()
    assert padder._pad[2] > 0 and padder._pad[0] > 0                      # padded on top and on the left
    res = metrics.FlowMetrics().update(t(pred), t(gt), None, t(noc), padder=padder).compute()
    assert res['skipped'] == 0
    for key in ('epe', '1px', '3px', '5px', 's0_10', 's10_40', 's40+', 'matched', 'unmatched'):
        check_result(key, res[key], golden[f'sintel/sintel_{dstype}_{key}'], f'sintel {dstype} ')
    # float64 means of the same float32 per-pixel values
    crop = (padder._pad[2], padder._pad[0])
    px = [flow_pixels(pred[i], gt[i], crop) for i in range(N)]
    check_sum(res['epe'], mean64([e for e, _ in px]), 'epe f64', REL_FLOAT64)
    for key, sel in (('s0_10', lambda m: m < 10), ('s10_40', lambda m: (m >= 10) & (m <= 40)), ('s40+', lambda m: m > 40)):
        assert all(sel(m).any() for _, m in px)                         # every bin of every sample is populated
        check_sum(res[key], mean64([e[sel(m)] for e, m in px]), key + ' f64', REL_FLOAT64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    matched = [(noc[i] > 0.5) & (xs + gt[i, 0] >= 0) & (xs + gt[i, 0] <= W - 1) & (ys + gt[i, 1] >= 0) & (ys + gt[i, 1] <= H - 1)
               & (np.abs(gt[i, 0]) <= W - 1) & (np.abs(gt[i, 1]) <= H - 1) for i in range(N)]
    assert all(m.any() and (~m).any() for m in matched)
    check_sum(res['matched'], mean64([px[i][0][matched[i]] for i in range(N)]), 'matched f64', REL_FLOAT64)
    check_sum(res['unmatched'], mean64([px[i][0][~matched[i]] for i in range(N)]), 'unmatched f64', REL_FLOAT64)


@pytest.mark.parametrize('pixels', [True, False])
def test_kitti_results_match_the_reference(golden, pixels):
    pred, gt, valid = golden['kitti_pred'], golden['kitti_gt'], golden['kitti_valid']
    padder = kitti_padder()
    assert padder._pad[2] == 0 and padder._pad[3] > 0                     # all of the vertical padding at the bottom
    res = metrics.FlowMetrics().update(t(pred), t(gt), t(valid), padder=padder).compute(average_over_pixels=pixels)
    tag = 'kitti_pixels' if pixels else 'kitti_samples'
    assert 'matched' not in res and res['skipped'] == 0
    for key in ('epe', 'f1', 's0_10', 's10_40', 's40+'):
        check_result(key, res[key], golden[f'{tag}/kitti_{key}'], tag + ' ')
    px = [flow_pixels(pred[i], gt[i], (0, padder._pad[0])) for i in range(N)]
    val = [valid[i] >= 0.5 for i in range(N)]
    assert 0.1 < np.mean(val) < 0.6                                     # sparse
    pool = mean64 if pixels else (lambda parts: float(np.mean([np.mean(p.astype(np.float64)) for p in parts])))
    check_sum(res['epe'], pool([px[i][0][val[i]] for i in range(N)]), 'epe f64', REL_FLOAT64)
    for key, sel in (('s0_10', lambda m: m < 10), ('s10_40', lambda m: (m >= 10) & (m <= 40)), ('s40+', lambda m: m > 40)):
        check_sum(res[key], pool([px[i][0][val[i] & sel(px[i][1])] for i in range(N)]), key + ' f64', REL_FLOAT64)


def test_flow_fixture_covers_the_edge_cases(golden):
    assert str(golden['numpy_version'])
    for name in ('sintel_clean', 'sintel_final', 'kitti'):
        gt = golden[f'{name}_gt']
        mag = np.sqrt(gt[:, 0] ** 2 + gt[:, 1] ** 2)
        assert (mag == 0).any()                                          # epe / mag is inf or NaN there
        xs = np.arange(W, dtype=np.float32)
        assert ((xs + gt[:, 0]) < 0).any() and (np.abs(gt[:, 0]) > W - 1).any()      # targets out of frame, displacements too large
    rows = metrics.flow_rows_host(t(golden['kitti_pred']), t(golden['kitti_gt']), t(golden['kitti_valid']), None, (0, 1))
    assert (rows[:, [0, 6, 8, 10]] > 0).all()                           # no sample is wholly invalid, every speed bin of every sample is populated
    assert (rows[:, [2, 3, 4, 5]].sum(0) > 0).all() and (rows[:, [2, 3, 4, 5]].sum(0) < rows[:, 0].sum()).all()


def test_flow_sample_without_a_valid_pixel_is_skipped(golden):
    pred, gt, valid = t(golden['kitti_pred']), t(golden['kitti_gt']), t(golden['kitti_valid']).clone()
    full = metrics.FlowMetrics().update(pred[:3], gt[:3], valid[:3], padder=kitti_padder())
    valid[3] = 0
    part = metrics.FlowMetrics().update(pred, gt, valid, padder=kitti_padder())
    for mode in (True, False):
        a, b = full.compute(mode), part.compute(mode)
        assert b['skipped'] == 1 and a['skipped'] == 0
        assert {k: v for k, v in a.items() if k != 'skipped'} == {k: v for k, v in b.items() if k != 'skipped'}
    with pytest.raises(ValueError):
        part.update(pred, gt, valid, noc_valid=valid, padder=kitti_padder())         # noc_valid for some updates only


# ------------------------------------------------------------------ stereo and depth
@pytest.mark.parametrize('tag', ['all', 'things'])
def test_stereo_results_match_the_reference(golden, tag):
    pred, gt = t(golden['disp_pred']), t(golden['disp_gt'])
    max_disp = float(golden['disp_max_disp']) if tag == 'things' else 0.0
    acc = metrics.StereoMetrics(max_disp=max_disp).update(pred, gt)
    per = acc.per_sample()
    assert per.pop('skipped') == 0
    res = acc.compute()
    assert set(res) == {'epe', 'd1', 'thres1', 'thres2', 'thres3', 'bad', 'skipped'}
    for key, values in per.items():
        rec = golden[f'disp_{tag}/{key}']
        assert rec.max() > 0 and (key == 'epe' or rec.min() < 1), (key, rec)       # no share is degenerate over the set
        for i in range(N):
            check_result(key, float(values[i]), rec[i], f'disp {tag} [{i}] ')
        assert res[key] == float(np.mean(values))
    mask = (golden['disp_gt'] > 0) & ((golden['disp_gt'] < max_disp) if max_disp else True)
    e = np.abs(golden['disp_gt'] - golden['disp_pred'])
    assert e.dtype == np.float32
    for i in range(N):
        check_sum(float(per['epe'][i]), np.mean(e[i][mask[i]].astype(np.float64)), 'epe f64', REL_FLOAT64)


def test_stereo_sample_with_an_empty_mask_is_skipped(golden):
    pred, gt = t(golden['disp_pred']), t(golden['disp_gt']).clone()
    want = metrics.StereoMetrics().update(pred[1:], gt[1:]).compute()
    gt[0] = 0
    got = metrics.StereoMetrics().update(pred, gt).compute()
    assert got.pop('skipped') == 1 and want.pop('skipped') == 0 and got == want


def test_depth_results_match_the_reference(golden):
    lo, hi = (float(v) for v in golden['depth_range'])
    acc = metrics.DepthMetrics(lo, hi).update(t(golden['depth_pred']), t(golden['depth_gt']), t(golden['depth_valid']))
    per = acc.per_sample()
    assert per.pop('skipped') == 0
    res = acc.compute()
    assert set(res) == {'abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'skipped'}
    for key, values in per.items():
        for i in range(N):
            check_result(key, float(values[i]), golden[f'depth/{key}'][i], f'depth [{i}] ')
        assert res[key] == float(np.mean(values))
    d, p = golden['depth_gt'], golden['depth_pred']
    mask = (d > np.float32(lo)) & (d < np.float32(hi)) & (golden['depth_valid'] > 0.5)
    for i in range(N):
        g, q = d[i][mask[i]], p[i][mask[i]]
        sq = (g - q) * (g - q)
        assert sq.dtype == np.float32
        check_sum(float(per['abs_rel'][i]), np.mean((np.abs(g - q) / g).astype(np.float64)), 'abs_rel f64', REL_FLOAT64)
        check_sum(float(per['sq_rel'][i]), np.mean((sq / g).astype(np.float64)), 'sq_rel f64', REL_FLOAT64)
        check_sum(float(per['rmse'][i]), np.sqrt(np.mean(sq.astype(np.float64))), 'rmse f64', REL_FLOAT64)


def test_depth_thresholds_compare_in_float32():
    """``thresh < 1.25 ** 2``: a weak Python scalar under NumPy 2, an exactly representable one under NumPy 1 -- a float32 comparison
    either way, so a ratio one float32 step below 1.5625 counts and 1.5625 itself does not."""
    below = np.nextafter(np.float32(1.5625), np.float32(0))
    gt = torch.tensor([[[1.0, 1.0, 1.0, 1.0]]])
    pred = torch.tensor([[[float(below), 1.5625, 1.953125, float(np.nextafter(np.float32(1.953125), np.float32(0)))]]])
    rows = metrics.depth_rows_host(pred, gt)
    assert rows[0, [0, 5, 6, 7]].tolist() == [4, 0, 1, 3]
    assert (np.float32([below]) < 1.25 ** 2).all() and not (np.float32([1.5625]) < 1.25 ** 2).any()


# ------------------------------------------------------------------ batching and crops
def test_rows_do_not_depend_on_batching(golden):
    pred, gt, valid = t(golden['kitti_pred']), t(golden['kitti_gt']), t(golden['kitti_valid'])
    noc = t(golden['sintel_clean_noc'])
    whole = metrics.FlowMetrics().update(pred, gt, valid, noc, padder=kitti_padder())
    single = metrics.FlowMetrics()
    for i in range(N):
        single.update(pred[i:i + 1], gt[i:i + 1], valid[i:i + 1], noc[i:i + 1], padder=kitti_padder())
    assert np.array_equal(whole.rows(), single.rows()) and whole.compute() == single.compute()
    for cls, args in ((metrics.StereoMetrics, (t(golden['disp_pred']), t(golden['disp_gt']))),
                      (metrics.DepthMetrics, (t(golden['depth_pred']), t(golden['depth_gt']), t(golden['depth_valid'])))):
        a = cls().update(*args)
        b = cls()
        for i in range(N):
            b.update(*(x[i:i + 1] for x in args))
        assert np.array_equal(a.rows(), b.rows())


@pytest.mark.parametrize('mode', ['sintel', 'kitti'])
def test_padder_crop_equals_explicit_unpad(mode):
    pred, gt, valid, noc = seeded_flow_case(2, 37, 53, seed=7)
    padder = io.InputPadder((2, 3, 37, 53), mode=mode, padding_factor=8)
    padded = padder.pad(pred)[0] + 0.0
    padded[..., :padder._pad[2], :] = 1e6                                # whatever is in the padding must not matter
    padded[..., :, :padder._pad[0]] = -1e6
    padded[..., 37 + padder._pad[2]:, :] = float('nan')
    a = metrics.FlowMetrics().update(padded, gt, valid, noc, padder=padder).rows()
    b = metrics.FlowMetrics().update(padder.unpad(padded).contiguous(), gt, valid, noc).rows()
    assert np.array_equal(a, b) and np.isfinite(a).all()
    one = (padded[:, 0].abs() + 0.1).contiguous()
    for cls in (metrics.StereoMetrics, metrics.DepthMetrics):
        gt1 = gt[:, 0].abs() + 0.5
        assert np.array_equal(cls().update(one, gt1, padder=padder).rows(), cls().update(padder.unpad(one).contiguous(), gt1).rows())
    with pytest.raises(ValueError):
        metrics.FlowMetrics().update(padded, gt)                         # sizes differ and no padder
    with pytest.raises(ValueError):
        metrics.FlowMetrics().update(padded[..., 1:], gt, padder=padder)


# ------------------------------------------------------------------ validate_flow, readers, command line
class StubModel:
    """Returns the recorded padded predictions in call order, whatever the batch size."""

    def __init__(self, padded):
        self.padded, self.at, self.batches = padded, 0, []

    def __call__(self, image1, image2, **kw):
        assert kw['task'] == 'flow' and tuple(image1.shape[-2:]) == tuple(self.padded.shape[-2:])
        b = image1.shape[0]
        out = self.padded[self.at:self.at + b]
        self.at += b
        self.batches.append(b)
        return {'flow_preds': [torch.zeros_like(out), out]}


def kind(key):
    """The comparison rule of a result key: its own name for a share, 'epe' for every sum-type result."""
    last = key.rsplit('_', 1)[1]
    return last if last in SHARE_KEYS else 'epe'


def samples_of(gt, valid, noc=None):
    img = torch.zeros(3, H, W)
    for i in range(gt.shape[0]):
        yield (img, img, t(gt[i]), t(valid[i])) + ((t(noc[i]),) if noc is not None else ())


@pytest.mark.parametrize('batch_size', [1, 3])
def test_validate_flow_sintel_with_a_stub_model(golden, batch_size):
    stub = StubModel(t(golden['sintel_clean_pred']))
    res = evaluate.validate_flow(stub, samples_of(golden['sintel_clean_gt'], np.ones((N, H, W), np.float32), golden['sintel_clean_noc']),
                                 'sintel_clean', mode='sintel', with_speed_metric=True, evaluate_matched_unmatched=True,
                                 batch_size=batch_size, attn_type='swin')
    recorded = {k[len('sintel/'):]: golden[k] for k in golden.files if k.startswith('sintel/sintel_clean_')}
    assert set(res) == set(recorded) and all(isinstance(v, float) for v in res.values())
    assert stub.batches == ([1] * 4 if batch_size == 1 else [3, 1])
    for key, rec in recorded.items():
        check_result(kind(key), res[key], rec, key + ' ')
    plain = evaluate.validate_flow(StubModel(t(golden['sintel_clean_pred'])),
                                   samples_of(golden['sintel_clean_gt'], np.ones((N, H, W), np.float32)), 'x', mode='sintel')
    assert set(plain) == {'x_epe', 'x_1px', 'x_3px', 'x_5px'} and plain['x_epe'] == res['sintel_clean_epe']
    assert evaluate.summary_lines(res, 'sintel_clean', 'Sintel (clean)')[0].startswith('Validation Sintel (clean) EPE: 4.615, 1px: 0.689')


@pytest.mark.parametrize('pixels', [True, False])
def test_validate_flow_kitti_with_a_stub_model(golden, pixels):
    res = evaluate.validate_flow(StubModel(t(golden['kitti_pred'])), samples_of(golden['kitti_gt'], golden['kitti_valid']), 'kitti',
                                 mode='kitti', with_speed_metric=True, average_over_pixels=pixels, batch_size=2)
    tag = 'kitti_pixels/' if pixels else 'kitti_samples/'
    recorded = {k[len(tag):]: golden[k] for k in golden.files if k.startswith(tag)}
    assert set(res) == set(recorded) == {'kitti_epe', 'kitti_f1', 'kitti_s0_10', 'kitti_s10_40', 'kitti_s40+'}
    for key, rec in recorded.items():
        check_result(kind(key), res[key], rec, key + ' ')
    with pytest.raises(ValueError):
        evaluate.validate_flow(StubModel(t(golden['kitti_pred'])), [], 'kitti', mode='things')
    with pytest.raises(ValueError):                                     # matched / unmatched without noc_valid in the samples
        evaluate.validate_flow(StubModel(t(golden['kitti_pred'])), samples_of(golden['kitti_gt'], golden['kitti_valid']), 'k',
                               evaluate_matched_unmatched=True)


def test_mixed_sizes_are_grouped_by_size():
    calls = []

    def model(image1, image2, **kw):
        calls.append(tuple(image1.shape))
        return {'flow_preds': [torch.zeros(image1.shape[0], 2, *image1.shape[-2:])]}
    sizes = [(16, 24), (16, 24), (16, 24), (13, 24), (16, 24)]
    samples = [(torch.zeros(3, h, w), torch.zeros(3, h, w), torch.ones(2, h, w), torch.ones(h, w)) for h, w in sizes]
    res = evaluate.validate_flow(model, samples, 'p', batch_size=2)
    assert calls == [(2, 3, 16, 24), (1, 3, 16, 24), (1, 3, 16, 24), (1, 3, 16, 24)]
    assert res['p_epe'] == pytest.approx(2 ** 0.5, rel=1e-7) and res['p_1px'] == 1.0 and res['p_3px'] == 0.0


def test_dataset_readers_roundtrip(tmp_path):
    pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(3)
    h, w = 12, 20
    sintel = tmp_path / 'Sintel'
    frames, flows, occs = {}, {}, {}
    for scene, count in (('alley_1', 3), ('bamboo_2', 2)):
        for sub in ('clean', 'flow', 'occlusions'):
            os.makedirs(sintel / 'training' / sub / scene)
        for i in range(count):
            frames[scene, i] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            io.write_png8(sintel / 'training' / 'clean' / scene / ('frame_%04d.png' % (i + 1)), frames[scene, i])
        for i in range(count - 1):
            flows[scene, i] = rng.normal(0, 5, (h, w, 2)).astype(np.float32)
            flows[scene, i][0, 0] = (2000.0, 0.0)                        # invalid by the |u| < 1000 rule
            occs[scene, i] = (rng.random((h, w)) < 0.3).astype(np.uint8) * 255
            io.write_flo(sintel / 'training' / 'flow' / scene / ('frame_%04d.flo' % (i + 1)), flows[scene, i])
            io.write_png8(sintel / 'training' / 'occlusions' / scene / ('frame_%04d.png' % (i + 1)), occs[scene, i])
    pairs = evaluate.SintelPairs(str(sintel), 'clean', load_occlusion=True)
    assert len(pairs) == 3
    order = [('alley_1', 0), ('alley_1', 1), ('bamboo_2', 0)]
    for item, (scene, i) in zip(pairs, order):
        img1, img2, flow, valid, noc = item
        assert img1.dtype == torch.float32 and np.array_equal(img1.permute(1, 2, 0).numpy(), frames[scene, i].astype(np.float32))
        assert np.array_equal(img2.permute(1, 2, 0).numpy(), frames[scene, i + 1].astype(np.float32))
        assert np.array_equal(flow.permute(1, 2, 0).numpy(), flows[scene, i])
        assert valid[0, 0] == 0 and valid.sum() == h * w - 1
        assert np.array_equal(noc.numpy(), 1 - occs[scene, i].astype(np.float32) / 255)
    assert len(evaluate.SintelPairs(str(sintel), 'clean')[0]) == 4
    with pytest.raises(FileNotFoundError):
        evaluate.SintelPairs(str(sintel), 'final')

    kitti = tmp_path / 'KITTI'
    os.makedirs(kitti / 'training' / 'image_2')
    os.makedirs(kitti / 'training' / 'flow_occ')
    uv, val = {}, {}
    for i in range(2):
        for j in (10, 11):
            frames[i, j] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            io.write_png8(kitti / 'training' / 'image_2' / ('%06d_%d.png' % (i, j)), frames[i, j])
        uv[i] = np.round(rng.normal(0, 20, (h, w, 2)) * 64) / 64              # representable in the 1/64 px encoding
        val[i] = (rng.random((h, w)) < 0.4)
        png = np.concatenate([64.0 * uv[i] + 2 ** 15, val[i][..., None].astype(np.float64)], -1).astype(np.uint16)
        io.write_png16(kitti / 'training' / 'flow_occ' / ('%06d_10.png' % i), png)
    pairs = evaluate.KittiPairs(str(kitti))
    assert len(pairs) == 2
    for i, (img1, img2, flow, valid) in enumerate(pairs):
        assert np.array_equal(img1.permute(1, 2, 0).numpy(), frames[i, 10].astype(np.float32))
        assert np.array_equal(img2.permute(1, 2, 0).numpy(), frames[i, 11].astype(np.float32))
        assert np.array_equal(flow.permute(1, 2, 0).numpy(), uv[i].astype(np.float32)) and np.array_equal(valid.numpy() > 0.5, val[i])


def test_command_line_arguments():
    args = evaluate.build_parser().parse_args(['--dataset', 'kitti', '--root', '/data/KITTI', '--per-sample', '--batch-size', '4',
                                               '--with-speed-metric', '--weights', 'w.pth'])
    assert (args.dataset, args.root, args.per_sample, args.batch_size, args.with_speed_metric) == ('kitti', '/data/KITTI', True, 4, True)
    assert args.model_config == 'gmflow_s1' and args.precision == 'exact' and args.weights == 'w.pth' and args.padding_factor == 8
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(['--dataset', 'chairs', '--root', 'x'])
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(['--dataset', 'sintel'])


# ------------------------------------------------------------------ C ABI without a GPU
NAMES = ('um_flow_metrics', 'um_disp_metrics', 'um_depth_metrics')


def test_metric_symbols_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'unimatch_hip.h')).read()
    for name in NAMES + tuple(n + '_workspace_bytes' for n in NAMES):
        assert f'{name}(' in text and hasattr(lib, name) and name in _abi.SIGNATURES
    assert (metrics.FLOW_K, metrics.DISP_K, metrics.DEPTH_K) == (16, 8, 8)
    for name, k in (('FLOW', 16), ('DISP', 8), ('DEPTH', 8)):
        assert f'#define UM_{name}_METRICS_K {k}' in text


def test_metric_abi_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(64)
    big = 1 << 20
    # one partial row per 2048 pixels and sample
    assert lib.um_flow_metrics_workspace_bytes(2, 436, 1024) == 2 * 218 * 16 * 8
    assert lib.um_disp_metrics_workspace_bytes(1, 37, 53) == 1 * 1 * 8 * 8
    assert lib.um_depth_metrics_workspace_bytes(3, 64, 65) == 3 * 3 * 8 * 8
    for q in (lib.um_flow_metrics_workspace_bytes, lib.um_disp_metrics_workspace_bytes, lib.um_depth_metrics_workspace_bytes):
        assert q(0, 8, 8) == 0 and q(1, 0, 8) == 0 and q(1, 8, -1) == 0

    def flow(pred=p, gt=p, rows=p, b=1, hp=40, wp=56, h=37, w=53, top=1, left=1, ws=p, nbytes=big):
        return lib.um_flow_metrics(pred, gt, None, None, rows, b, hp, wp, h, w, top, left, ws, nbytes, None)

    def disp(pred=p, gt=p, rows=p, b=1, hp=40, wp=56, h=37, w=53, top=1, left=1, ws=p, nbytes=big):
        return lib.um_disp_metrics(pred, gt, rows, b, hp, wp, h, w, top, left, 0.0, ws, nbytes, None)

    def depth(pred=p, gt=p, rows=p, b=1, hp=40, wp=56, h=37, w=53, top=1, left=1, ws=p, nbytes=big):
        return lib.um_depth_metrics(pred, gt, None, rows, b, hp, wp, h, w, top, left, 0.0, 10.0, ws, nbytes, None)

    for call in (flow, disp, depth):
        assert call(pred=None) == -1 and call(gt=None) == -1 and call(rows=None) == -1          # null pointers
        assert call(b=0) == -1 and call(h=0) == -1 and call(w=-3) == -1 and call(hp=0) == -1     # non-positive sizes
        assert call(top=4) == -1 and call(left=4) == -1 and call(top=-1) == -1 and call(left=-1) == -1   # crop leaves the frame
        assert call(hp=36) == -1 and call(wp=52) == -1
        assert b'crop' in lib.um_last_error_string()
        assert call(ws=None) == -3 and call(nbytes=8) == -3                                      # workspace
        assert b'workspace' in lib.um_last_error_string()
