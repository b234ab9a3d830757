"""Evaluation-loop cost of the flow metrics: the reference's host path against the device-side accumulators.

    python tools/bench_metrics.py [--out profiles/metrics_eval.txt] [--samples 32] [--pairs 12]

At 436 x 1024 (Sintel, InputPadder mode 'sintel') and 375 x 1242 (KITTI, mode 'kitti', sparse valid), batch 1, padding factor 16:

  metrics only, over ``--samples`` already-computed padded predictions that live on the device
    host      what the reference does per sample: ``padder.unpad(flow_pr[0]).cpu()`` and the statistics on the host (the project's host
              restatement, which is written in the reference's operations)
    copy      the ``.cpu()`` of that path alone (device-to-host copy of 8 B/px and the synchronisation it implies)
    device    ``FlowMetrics.update`` per sample on the device, one ``compute()`` at the end
  whole loop, ``--pairs`` synthetic pairs through gmflow_s1 (seeded weights)
    host_loop     forward, ``.cpu()``, host statistics per pair (the reference's loop)
    validate_flow ``unimatch_amd.evaluate.validate_flow``

Every figure is the median of 5 synchronised regions (synchronize, wall clock, synchronize) after a warm-up of every leg, the legs
alternating inside one process; ms per sample.  The traffic floor of the metric kernels is 20-24 B/px.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import UniMatch  # noqa: E402
from unimatch_amd.evaluate import validate_flow  # noqa: E402
from unimatch_amd.io import InputPadder  # noqa: E402
from unimatch_amd.metrics import FlowMetrics  # noqa: E402
from unimatch_amd.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 5
PADDING = 16                  # the reference's scale-1 evaluation scripts: features at 1/8 must split in two for the Swin attention


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns):
    for fn in fns.values():                            # warm-up of every leg
        fn()
    times = {k: [] for k in fns}
    for _ in range(REGIONS):
        for k, fn in fns.items():
            times[k].append(region(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def case(h, w, mode, samples):
    g = torch.Generator().manual_seed(h)
    gt = (torch.randn(samples, 2, h, w, generator=g) * 12).float()
    pred = gt + torch.randn(samples, 2, h, w, generator=g) * 2
    valid = (torch.rand(samples, h, w, generator=g) < (0.3 if mode == 'kitti' else 1.1)).float()
    padder = InputPadder((1, 3, h, w), mode=mode, padding_factor=PADDING)
    padded = padder.pad(pred)[0].contiguous()
    return padder, padded, gt, valid


def metrics_rows(h, w, mode, samples, lines):
    padder, padded, gt, valid = case(h, w, mode, samples)
    use_valid = mode == 'kitti'
    dev_pred, dev_gt, dev_valid = padded.cuda(), gt.cuda(), valid.cuda()
    results = {}

    def host():
        acc = FlowMetrics()
        for i in range(samples):
            flow = padder.unpad(dev_pred[i]).cpu()
            acc.update(flow[None], gt[i:i + 1], valid[i:i + 1] if use_valid else None)
        results['host'] = acc.compute()

    def copy():
        for i in range(samples):
            padder.unpad(dev_pred[i]).cpu()

    def device():
        acc = FlowMetrics()
        for i in range(samples):
            acc.update(dev_pred[i:i + 1], dev_gt[i:i + 1], dev_valid[i:i + 1] if use_valid else None, padder=padder)
        results['device'] = acc.compute()

    t = alternate({'host': host, 'copy': copy, 'device': device})
    a, b = results['host'], results['device']
    assert all(abs(a[k] - b[k]) <= 1e-12 * abs(a[k]) for k in a if k != 'skipped'), (a, b)
    lines.append(f'metrics only, {h} x {w}, InputPadder {mode}, batch 1, {samples} predictions per region (ms per sample: median [min .. max])')
    for k in ('host', 'copy', 'device'):
        med, lo, hi = (1e3 * x / samples for x in t[k])
        lines.append(f'  {k:<14}{med:9.4f}  [{lo:.4f} .. {hi:.4f}]')
    lines.append(f'  host / device {t["host"][0] / t["device"][0]:9.1f} x     (epe {b["epe"]:.6f} on both paths)')


def loop_rows(h, w, mode, pairs, lines):
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}))
    model = model.cuda()
    kw = {k: v for k, v in fk.items() if k != 'task'}
    data = []
    for i in range(pairs):
        i1, i2 = synth_images(1, h, w, seed=900 + i, kind='shift')
        gt = torch.tensor([-6.0, 4.0]).view(2, 1, 1).expand(2, h, w).contiguous()
        valid = (torch.rand(h, w, generator=torch.Generator().manual_seed(i)) < (0.3 if mode == 'kitti' else 1.1)).float()
        data.append((i1[0].cuda(), i2[0].cuda(), gt, valid))
    on_device = [(a, b, gt.cuda(), valid.cuda()) for a, b, gt, valid in data]
    results = {}

    def host_loop():
        acc = FlowMetrics()
        for i1, i2, gt, valid in data:
            padder = InputPadder(i1[None].shape, mode=mode, padding_factor=PADDING)
            a, b = padder.pad(i1[None], i2[None])
            with torch.no_grad():
                flow_pr = model(a, b, task='flow', **kw)['flow_preds'][-1]
            flow = padder.unpad(flow_pr[0]).cpu()
            acc.update(flow[None], gt[None], valid[None] if mode == 'kitti' else None)
        results['host_loop'] = acc.compute()['epe']

    def device_loop():
        results['validate_flow'] = validate_flow(model, on_device, 'x', mode=mode, padding_factor=PADDING, **kw)['x_epe']

    t = alternate({'host_loop': host_loop, 'validate_flow': device_loop})
    assert abs(results['host_loop'] - results['validate_flow']) <= 1e-12 * abs(results['host_loop']), results
    lines.append(f'whole loop, gmflow_s1 exact, {h} x {w}, InputPadder {mode}, batch 1, {pairs} pairs per region (ms per pair: median [min .. max])')
    for k in ('host_loop', 'validate_flow'):
        med, lo, hi = (1e3 * x / pairs for x in t[k])
        lines.append(f'  {k:<14}{med:9.4f}  [{lo:.4f} .. {hi:.4f}]')
    lines.append(f'  host_loop / validate_flow {t["host_loop"][0] / t["validate_flow"][0]:6.3f} x')
    del model
    torch.cuda.empty_cache()


def main():
    if not torch.cuda.is_available():
        raise SystemExit('no GPU visible: nothing is measured without one')
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'metrics_eval.txt'))
    samples, pairs = arg('--samples', 32), arg('--pairs', 12)
    lines = [f'tools/bench_metrics.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'median of {REGIONS} synchronised regions per leg, legs alternating in one process, every leg warmed up once', '']
    for h, w, mode in ((436, 1024, 'sintel'), (375, 1242, 'kitti')):
        metrics_rows(h, w, mode, samples, lines)
        lines.append('')
        print('\n'.join(lines[-6:]), flush=True)
    for h, w, mode in ((436, 1024, 'sintel'), (375, 1242, 'kitti')):
        loop_rows(h, w, mode, pairs, lines)
        lines.append('')
        print('\n'.join(lines[-5:]), flush=True)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
