"""GPU tests of the evaluation metrics: ``um_flow_metrics`` / ``um_disp_metrics`` / ``um_depth_metrics`` against the host restatement
(count accumulators exactly, sum accumulators to 1e-12: the addends are the same float32 values, only the order of the float64
additions differs) and against the results recorded from the reference (tests/golden/metrics.npz; rules in tests/metrics_util.py),
determinism, NaN / inf, no host synchronisation in ``update``, and ``validate_flow`` end to end."""
import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, evaluate, io, metrics
from unimatch_amd.ops import KernelTimer
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_images, synth_state_dict
from tests.metrics_util import (DEPTH_COUNT_COLS, DEPTH_SUM_COLS, DISP_COUNT_COLS, DISP_SUM_COLS, FLOW_COUNT_COLS, FLOW_SUM_COLS,
                                SHARE_KEYS, check_result, check_rows, load_golden, seeded_flow_case)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, H, W = 4, 37, 53


@pytest.fixture(scope='module')
def golden():
    return load_golden()


def host(a):
    return torch.from_numpy(np.asarray(a))


def both(cls, args, kwargs=None, init=()):
    """The accumulator fed on the device and on the host with the same tensors."""
    kwargs = kwargs or {}
    on_dev = cls(*init).update(*(None if a is None else a.to(DEV) for a in args), **kwargs)
    on_host = cls(*init).update(*args, **kwargs)
    return on_dev, on_host


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize('name', ['sintel_clean', 'sintel_final', 'kitti'])
def test_flow_kernel_on_the_fixture(golden, name):
    kitti = name == 'kitti'
    padder = io.InputPadder((1, 3, H, W), mode='kitti' if kitti else 'sintel', padding_factor=8)
    args = (host(golden[f'{name}_pred']), host(golden[f'{name}_gt']), host(golden['kitti_valid']) if kitti else None,
            None if kitti else host(golden[f'{name}_noc']))
    got, want = both(metrics.FlowMetrics, args, {'padder': padder})
    check_rows(got.rows(), want.rows(), FLOW_COUNT_COLS, FLOW_SUM_COLS, name)
    if kitti:
        for tag, pixels in (('kitti_pixels', True), ('kitti_samples', False)):
            res = got.compute(average_over_pixels=pixels)
            for key in ('epe', 'f1', 's0_10', 's10_40', 's40+'):
                check_result(key, res[key], golden[f'{tag}/kitti_{key}'], tag + ' ')
    else:
        res = got.compute()
        for key in ('epe', '1px', '3px', '5px', 's0_10', 's10_40', 's40+', 'matched', 'unmatched'):
            check_result(key, res[key], golden[f'sintel/{name}_{key}'], name + ' ')


@pytest.mark.parametrize('tag', ['all', 'things'])
def test_disp_kernel_on_the_fixture(golden, tag):
    max_disp = float(golden['disp_max_disp']) if tag == 'things' else 0.0
    got, want = both(metrics.StereoMetrics, (host(golden['disp_pred']), host(golden['disp_gt'])), init=(max_disp,))
    check_rows(got.rows(), want.rows(), DISP_COUNT_COLS, DISP_SUM_COLS, 'disp ' + tag)
    per = got.per_sample()
    assert per.pop('skipped') == 0
    for key, values in per.items():
        for i in range(N):
            check_result(key, float(values[i]), golden[f'disp_{tag}/{key}'][i], f'disp {tag} [{i}] ')


def test_depth_kernel_on_the_fixture(golden):
    lo, hi = (float(v) for v in golden['depth_range'])
    got, want = both(metrics.DepthMetrics, (host(golden['depth_pred']), host(golden['depth_gt']), host(golden['depth_valid'])),
                     init=(lo, hi))
    check_rows(got.rows(), want.rows(), DEPTH_COUNT_COLS, DEPTH_SUM_COLS, 'depth')
    per = got.per_sample()
    assert per.pop('skipped') == 0
    for key, values in per.items():
        for i in range(N):
            check_result(key, float(values[i]), golden[f'depth/{key}'][i], f'depth [{i}] ')


# ------------------------------------------------------------------ seeded inputs at evaluation sizes
@pytest.mark.parametrize('b,h,w,mode', [(1, 436, 1024, 'sintel'), (1, 436, 1024, 'kitti'), (1, 375, 1242, 'sintel'),
                                        (1, 375, 1242, 'kitti'), (8, 512, 768, 'sintel')])
def test_flow_kernel_against_the_host_restatement(b, h, w, mode):
    pred, gt, valid, noc = seeded_flow_case(b, h, w, seed=h + w + b, sparse=mode == 'kitti')
    padder = io.InputPadder((b, 3, h, w), mode=mode, padding_factor=8 if b == 1 else 32)
    padded = padder.pad(pred)[0].contiguous()
    assert (h, w) == (512, 768) or tuple(padded.shape[-2:]) != (h, w)
    for use_valid, use_noc in ((True, True), (False, False), (True, False), (False, True)):
        args = (padded, gt, valid if use_valid else None, noc if use_noc else None)
        got, want = both(metrics.FlowMetrics, args, {'padder': padder})
        check_rows(got.rows(), want.rows(), FLOW_COUNT_COLS, FLOW_SUM_COLS, f'{b}x{h}x{w} {mode} valid={use_valid} noc={use_noc}')
        for pixels in (True, False):
            a, c = got.compute(pixels), want.compute(pixels)
            assert set(a) == set(c) and a['skipped'] == c['skipped'] == 0
            for key in a:
                if key in SHARE_KEYS:
                    assert a[key] == c[key], key
                elif key != 'skipped':
                    assert abs(a[key] - c[key]) <= 1e-12 * abs(c[key]), (key, a[key], c[key])
        if b > 1:                                                        # a sample's row does not depend on its batch
            alone = metrics.FlowMetrics().update(padded[3:4].to(DEV), gt[3:4].to(DEV), None if not use_valid else valid[3:4].to(DEV),
                                                 None if not use_noc else noc[3:4].to(DEV), padder=padder)
            assert np.array_equal(alone.rows()[0], got.rows()[3])


@pytest.mark.parametrize('h,w,mode', [(375, 1242, 'kitti'), (436, 1024, 'sintel')])
def test_disp_and_depth_kernels_against_the_host_restatement(h, w, mode):
    g = torch.Generator().manual_seed(h)
    b = 2
    padder = io.InputPadder((b, 3, h, w), mode=mode, padding_factor=32)
    disp = (torch.rand(b, h, w, generator=g) * 190.0).float()
    disp[:, :7] = 0.0
    disp[:, 7:9] *= 0.004
    est = padder.pad((disp + torch.randn(b, h, w, generator=g) * 4.0 * torch.rand(b, h, w, generator=g)).float())[0].contiguous()
    for max_disp in (0.0, 150.0):
        got, want = both(metrics.StereoMetrics, (est, disp), {'padder': padder}, init=(max_disp,))
        check_rows(got.rows(), want.rows(), DISP_COUNT_COLS, DISP_SUM_COLS, f'disp {h}x{w} max_disp={max_disp}')
    depth = (0.2 + 11.0 * torch.rand(b, h, w, generator=g)).float()
    pred = padder.pad((depth * torch.exp(0.3 * torch.randn(b, h, w, generator=g))).float())[0].contiguous()
    valid = (torch.rand(b, h, w, generator=g) > 0.2).float()
    for v in (valid, None):
        got, want = both(metrics.DepthMetrics, (pred, depth, v), {'padder': padder}, init=(0.5, 10.0))
        check_rows(got.rows(), want.rows(), DEPTH_COUNT_COLS, DEPTH_SUM_COLS, f'depth {h}x{w} valid={v is not None}')


# ------------------------------------------------------------------ determinism, NaN / inf
def test_rows_are_bitwise_reproducible_and_the_workspace_is_stateless():
    """Two calls give bitwise-equal rows; so does a call after another geometry used the SAME workspace memory (the C ABI is called
    directly with one buffer that every call shares)."""
    lib = _abi.load()
    pa, ga, va, na = (x.to(DEV) for x in seeded_flow_case(2, 436, 1024, seed=31))
    pb, gb, vb, nb = (x.to(DEV) for x in seeded_flow_case(3, 200, 333, seed=32))
    ws = torch.full((1 << 20,), 0x7f, dtype=torch.uint8, device=DEV)      # starts as garbage (NaN patterns), never cleared
    stream = torch.cuda.current_stream().cuda_stream

    def run(p, g, v, n):
        b, _, h, w = g.shape
        assert lib.um_flow_metrics_workspace_bytes(b, h, w) <= ws.numel()
        rows = torch.empty(b, 16, dtype=torch.float64, device=DEV)
        _abi.check(lib.um_flow_metrics(p.data_ptr(), g.data_ptr(), v.data_ptr(), n.data_ptr(), rows.data_ptr(), b, h, w, h, w, 0, 0,
                                       ws.data_ptr(), ws.numel(), stream), 'um_flow_metrics')
        return rows

    first = run(pa, ga, va, na)
    again = run(pa, ga, va, na)
    other = run(pb, gb, vb, nb)
    after = run(pa, ga, va, na)
    torch.cuda.synchronize()
    assert torch.equal(first, again) and torch.equal(first, after)
    assert torch.isfinite(first).all() and torch.isfinite(other).all()
    want = metrics.flow_rows_host(pb.cpu(), gb.cpu(), vb.cpu(), nb.cpu())
    check_rows(other.cpu().numpy(), want.numpy(), FLOW_COUNT_COLS, FLOW_SUM_COLS, 'shared workspace')
    # through the wrappers: the same rows as the direct call
    assert torch.equal(metrics._hip().flow_metrics(pa, ga, va, na), first)


def test_nan_and_inf_predictions_behave_as_on_the_host():
    pred, gt, valid, noc = seeded_flow_case(3, 64, 96, seed=41)
    valid[:] = 1.0
    pred[0, 0, 10, 10] = float('nan')                                   # mag < 10 there: that bin's sum is NaN, the others are not
    pred[1, 1, 20, 90] = float('inf')
    pred[2, 0, 6, 4] = float('inf')                                     # where nothing moves: inf / 0
    got, want = both(metrics.FlowMetrics, (pred, gt, valid, noc))
    g, w_ = got.rows(), want.rows()
    check_rows(g, w_, FLOW_COUNT_COLS, FLOW_SUM_COLS, 'nan / inf')
    assert np.isnan(g[0, 1]) and np.isinf(g[1, 1]) and np.isinf(g[2, 1])
    assert np.isnan(g[0, [7, 9, 11]]).sum() == 1 and np.isfinite(g[0, [7, 9, 11]]).sum() == 2
    clean = pred.clone()
    clean[0, :, 10, 10] = gt[0, :, 10, 10]
    ref = metrics.flow_rows_host(clean, gt, valid, noc)
    assert g[0, 2] == ref[0, 2].item() and g[0, 0] == ref[0, 0].item()    # a NaN pixel counts as a pixel and fails every comparison


# ------------------------------------------------------------------ update() does not wait for the GPU
def test_update_enqueues_one_launch_and_never_synchronises():
    """Checked two ways: the launch census of ``KernelTimer`` (one ``flow_metrics`` entry per update, nothing else), and torch's
    synchronisation debug mode, under which any device-to-host copy or stream wait raises."""
    pred, gt, valid, noc = (x.to(DEV) for x in seeded_flow_case(2, 125, 189, seed=51))
    padder = io.InputPadder((2, 3, 125, 189), padding_factor=8)
    padded = padder.pad(pred)[0].contiguous()
    ops = metrics._hip()
    acc = metrics.FlowMetrics().update(padded, gt, valid, noc, padder=padder)           # library, allocator warm
    torch.cuda.synchronize()
    ops.timer = KernelTimer()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                             # the mode does catch a synchronising call
        for _ in range(3):
            acc.update(padded, gt, valid, noc, padder=padder)
        records = list(ops.timer.records)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        ops.timer = None
    assert [r[0] for r in records] == ['flow_metrics'] * 3
    rows = acc.rows()
    assert rows.shape == (8, 16) and np.array_equal(rows[:2], rows[6:])


# ------------------------------------------------------------------ end to end
def test_validate_flow_end_to_end():
    """gmflow_s1 over shifted-texture pairs at an odd size (padded to 128 x 192): the result equals the metrics computed on the host
    from the same model outputs copied back.  The second image shows the first one's content displaced by (-6, +4) px."""
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    h, w = 125, 189
    samples = []
    for seed in (600, 601, 602, 603, 604):
        i1, i2 = synth_images(1, h, w, seed=seed, kind='shift')
        gt = torch.tensor([-6.0, 4.0]).view(2, 1, 1).expand(2, h, w).contiguous()
        valid = (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 0.5).float()
        samples.append((i1[0], i2[0], gt, valid, 1 - valid))
    for mode in ('sintel', 'kitti'):
        res = evaluate.validate_flow(model, samples, 'syn', mode=mode, with_speed_metric=False, evaluate_matched_unmatched=mode == 'sintel',
                                     average_over_pixels=False, batch_size=1, **kw)
        ref = metrics.FlowMetrics()
        for i1, i2, gt, valid, noc in samples:
            padder = io.InputPadder((1, 3, h, w), mode=mode, padding_factor=8)
            a, b = padder.pad(i1[None].to(DEV), i2[None].to(DEV))
            assert tuple(a.shape[-2:]) == (128, 192)
            with torch.no_grad():
                flow = model(a, b, task='flow', **kw)['flow_preds'][-1]
            ref.update(flow.cpu(), gt[None], valid[None] if mode == 'kitti' else None, noc[None] if mode == 'sintel' else None, padder=padder)
        want = ref.compute(average_over_pixels=mode != 'kitti')
        assert set(res) == {'syn_' + k for k in (('epe', '1px', '3px', '5px', 'matched', 'unmatched') if mode == 'sintel' else ('epe', 'f1'))}
        for key, value in res.items():
            short = key[len('syn_'):]
            print(mode, key, value, want[short])
            assert np.isfinite(value)
            if short in SHARE_KEYS:
                assert value == want[short], key
            else:
                assert abs(value - want[short]) <= 1e-12 * abs(want[short]), (key, value, want[short])
    model.check_operand_range()
