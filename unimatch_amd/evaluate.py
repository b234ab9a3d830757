"""The reference's optical-flow validation loop (``validate_sintel`` / ``validate_kitti``, evaluate_flow.py:349-638) with the
metrics kept on the device.

  validate_flow(model, samples, prefix, mode=...)   pad, forward, feed ``flow_preds[-1]`` -- still padded -- to
                                                     :class:`unimatch_amd.metrics.FlowMetrics`; one read-back at the end
  SintelPairs(root, dstype) / KittiPairs(root)       readers over the reference's directory layouts (PIL for the images)

``python -m unimatch_amd.evaluate --dataset sintel|kitti --root DIR [--weights ...]`` prints the reference's summary lines.  Where the
reference copies every prediction to the host and synchronises after every forward, nothing here waits for the GPU until the result
is asked for.  Stereo and depth validation loops are not provided (their accumulators are: ``StereoMetrics``, ``DepthMetrics``).
"""
import argparse
import glob
import os

import numpy as np
import torch

from .io import InputPadder, read_flo, read_kitti_flow
from .metrics import FlowMetrics

MODES = ('sintel', 'kitti')


def _model_device(model, fallback):
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration, TypeError):
        return fallback


def validate_flow(model, samples, prefix, mode='sintel', padding_factor=8, with_speed_metric=False, evaluate_matched_unmatched=False,
                  average_over_pixels=True, batch_size=1, **forward_kw):
    """Evaluate ``model`` over ``samples``, an iterable of ``(image1, image2, flow_gt, valid[, noc_valid])`` tensors (``[3, H, W]``,
    ``[2, H, W]``, ``[H, W]``), and return the reference's result dict: ``<prefix>_epe`` and

      mode='sintel'   ``_1px``, ``_3px``, ``_5px`` over every pixel (validate_sintel ignores ``valid``), with
                      ``evaluate_matched_unmatched`` also ``_matched`` / ``_unmatched`` (the samples then carry ``noc_valid``);
      mode='kitti'    ``_f1`` over ``valid >= 0.5``; ``average_over_pixels=False`` gives validate_kitti's per-sample means;

    with ``with_speed_metric`` also ``_s0_10``, ``_s10_40``, ``_s40+``.  ``mode`` also selects the InputPadder's mode.  Consecutive
    samples of one size are grouped up to ``batch_size`` (results do not depend on the grouping: the accumulators are per sample).
    ``forward_kw`` goes to ``model(image1, image2, task='flow', ...)``."""
    if mode not in MODES:
        raise ValueError(f'mode must be one of {MODES}')
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1')
    forward_kw = dict(forward_kw)
    forward_kw['task'] = 'flow'
    metrics = FlowMetrics()
    group = []

    def flush():
        cols = [torch.stack(c, 0) for c in zip(*group)]
        group.clear()
        device = _model_device(model, cols[0].device)
        image1, image2, flow_gt, valid = (c.to(device, non_blocking=True) for c in cols[:4])
        noc_valid = None
        if evaluate_matched_unmatched:
            if len(cols) < 5:
                raise ValueError('evaluate_matched_unmatched needs samples with noc_valid')
            noc_valid = cols[4].to(device, non_blocking=True)
        padder = InputPadder(image1.shape, mode=mode, padding_factor=padding_factor)
        image1, image2 = padder.pad(image1, image2)
        with torch.no_grad():
            flow_pr = model(image1, image2, **forward_kw)['flow_preds'][-1]
        metrics.update(flow_pr, flow_gt, valid if mode == 'kitti' else None, noc_valid, padder)

    for sample in samples:
        sample = tuple(sample)
        if group and (len(group) == batch_size or sample[0].shape != group[0][0].shape):
            flush()
        group.append(sample)
    if group:
        flush()

    res = metrics.compute(average_over_pixels=average_over_pixels if mode == 'kitti' else True)
    names = ['epe'] + (['1px', '3px', '5px'] if mode == 'sintel' else ['f1'])
    if with_speed_metric:
        names += ['s0_10', 's10_40', 's40+']
    if evaluate_matched_unmatched:
        names += ['matched', 'unmatched']
    return {f'{prefix}_{k}': res[k] for k in names}


def summary_lines(results, prefix, title):
    """The reference's ``print`` lines for one result dict."""
    r = {k[len(prefix) + 1:]: v for k, v in results.items() if k.startswith(prefix + '_')}
    lines = []
    if 'f1' in r:
        lines.append('Validation %s EPE: %.3f, F1-all: %.3f' % (title, r['epe'], r['f1']))
    else:
        lines.append('Validation %s EPE: %.3f, 1px: %.3f, 3px: %.3f, 5px: %.3f' % (title, r['epe'], r['1px'], r['3px'], r['5px']))
    if 's0_10' in r:
        lines.append('Validation %s s0_10: %.3f, s10_40: %.3f, s40+: %.3f' % (title, r['s0_10'], r['s10_40'], r['s40+']))
    if 'matched' in r:
        lines.append('Validation %s matched epe: %.3f, unmatched epe: %.3f' % (title, r['matched'], r['unmatched']))
    return lines


# ------------------------------------------------------------------ readers over the reference's directory layouts
def _read_image(path):
    from .video import read_frame
    return read_frame(path)


class SintelPairs:
    """``training/<dstype>/<scene>/frame_*.png`` with ``training/flow/<scene>/*.flo`` (and ``training/occlusions/<scene>/*.png``
    with ``load_occlusion``) as ``(image1, image2, flow_gt, valid[, noc_valid])``: ``valid`` is ``|u|, |v| < 1000``, ``noc_valid``
    ``1 - occlusion / 255``, as the reference's dataset returns them."""

    def __init__(self, root, dstype='clean', load_occlusion=False):
        self.items = []
        image_root = os.path.join(root, 'training', dstype)
        if not os.path.isdir(image_root):
            raise FileNotFoundError(image_root)
        for scene in sorted(os.listdir(image_root)):
            images = sorted(glob.glob(os.path.join(image_root, scene, '*.png')))
            flows = sorted(glob.glob(os.path.join(root, 'training', 'flow', scene, '*.flo')))
            occs = sorted(glob.glob(os.path.join(root, 'training', 'occlusions', scene, '*.png'))) if load_occlusion else None
            if len(flows) != len(images) - 1 or (occs is not None and len(occs) != len(flows)):
                raise ValueError(f'{scene}: {len(images)} frames, {len(flows)} flows' + ('' if occs is None else f', {len(occs)} occlusion maps'))
            for i, flow in enumerate(flows):
                self.items.append((images[i], images[i + 1], flow, None if occs is None else occs[i]))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        img1, img2, flo, occ = self.items[index]
        flow = torch.from_numpy(read_flo(flo)).permute(2, 0, 1).float().contiguous()
        valid = ((flow[0].abs() < 1000) & (flow[1].abs() < 1000)).float()
        out = (_read_image(img1), _read_image(img2), flow, valid)
        if occ is not None:
            from PIL import Image
            occlusion = torch.from_numpy(np.array(Image.open(occ)).astype(np.float32))
            if occlusion.dim() == 3:
                occlusion = occlusion[..., 0]
            out += ((1 - occlusion / 255.).float(),)
        return out

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class KittiPairs:
    """``training/image_2/*_10.png`` / ``*_11.png`` with ``training/flow_occ/*_10.png`` (16-bit: flow and its sparse ``valid``)."""

    def __init__(self, root):
        base = os.path.join(root, 'training')
        first = sorted(glob.glob(os.path.join(base, 'image_2', '*_10.png')))
        second = sorted(glob.glob(os.path.join(base, 'image_2', '*_11.png')))
        flows = sorted(glob.glob(os.path.join(base, 'flow_occ', '*_10.png')))
        if not (len(first) == len(second) == len(flows)):
            raise ValueError(f'{base}: {len(first)} / {len(second)} images and {len(flows)} flows')
        self.items = list(zip(first, second, flows))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        img1, img2, png = self.items[index]
        flow, valid = read_kitti_flow(png)
        return (_read_image(img1), _read_image(img2), torch.from_numpy(flow).permute(2, 0, 1).float().contiguous(),
                torch.from_numpy(valid).float())

    def __iter__(self):
        return (self[i] for i in range(len(self)))


# ------------------------------------------------------------------ command line
def build_parser():
    from .synth import CONFIGS
    ap = argparse.ArgumentParser(description="optical-flow validation on the reference's Sintel / KITTI layouts, metrics on the device")
    ap.add_argument('--dataset', required=True, choices=MODES)
    ap.add_argument('--root', required=True, help='dataset directory (the one that holds training/)')
    ap.add_argument('--padding-factor', type=int, default=8)
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--with-speed-metric', action='store_true')
    ap.add_argument('--evaluate-matched-unmatched', action='store_true', help='Sintel only: reads training/occlusions')
    ap.add_argument('--per-sample', action='store_true', help="KITTI only: validate_kitti's average_over_pixels=False")
    ap.add_argument('--model-config', default='gmflow_s1', choices=[k for k, v in CONFIGS.items() if v[1].get('task') == 'flow'])
    ap.add_argument('--weights', default=None, help="checkpoint (the reference's: a state_dict, or {'model': state_dict}); "
                                                    'default: the seeded synthetic weights')
    ap.add_argument('--precision', default='exact', choices=['exact', 'fast'])
    return ap


def main(argv=None):
    from .model import UniMatch
    from .synth import CONFIGS, synth_state_dict
    args = build_parser().parse_args(argv)
    ck, fk = CONFIGS[args.model_config]
    model = UniMatch(**ck).eval()
    if args.weights:
        sd = torch.load(args.weights, map_location='cpu')
        sd = sd.get('model', sd)
    else:
        sd = synth_state_dict({k: v.shape for k, v in model.state_dict().items()})
    model.load_state_dict(sd)
    model = model.to('cuda').set_precision(args.precision)
    fwd_kw = {k: v for k, v in fk.items() if k != 'task'}
    common = dict(padding_factor=args.padding_factor, with_speed_metric=args.with_speed_metric, batch_size=args.batch_size, **fwd_kw)
    results = {}
    if args.dataset == 'sintel':
        for dstype in ('clean', 'final'):
            pairs = SintelPairs(args.root, dstype, load_occlusion=args.evaluate_matched_unmatched)
            print('Number of validation image pairs: %d' % len(pairs))
            res = validate_flow(model, pairs, 'sintel_' + dstype, mode='sintel',
                                evaluate_matched_unmatched=args.evaluate_matched_unmatched, **common)
            print('\n'.join(summary_lines(res, 'sintel_' + dstype, 'Sintel (%s)' % dstype)))
            results.update(res)
    else:
        pairs = KittiPairs(args.root)
        print('Number of validation image pairs: %d' % len(pairs))
        results = validate_flow(model, pairs, 'kitti', mode='kitti', average_over_pixels=not args.per_sample, **common)
        print('\n'.join(summary_lines(results, 'kitti', 'KITTI')))
    return results


if __name__ == '__main__':
    main()
