"""The reference's validation loops with the metrics kept on the device.

  validate_flow(model, samples, prefix, mode=...)   ``validate_sintel`` / ``validate_kitti`` (evaluate_flow.py:349-638): pad, forward,
                                                     feed ``flow_preds[-1]`` -- still padded -- to
                                                     :class:`unimatch_amd.metrics.FlowMetrics`; one read-back at the end
  validate_stereo(model, samples, prefix, ...)      ``validate_things`` / ``validate_kitti15`` (evaluate_stereo.py:301-512)
  validate_depth(model, samples, prefix, ...)       ``validate_scannet`` (evaluate_depth.py:21-154)
  SintelPairs(root, dstype) / KittiPairs(root)       readers over the reference's directory layouts (PIL for the images)
  Kitti15StereoPairs(root)                           KITTI-2015 stereo: uint8 frames, normalised on the device

The stereo and depth loops pad or resize through :class:`unimatch_amd.prepost.InferenceGeometry` (``inference_size``), on the device.
``python -m unimatch_amd.evaluate --dataset sintel|kitti|kitti15-stereo --root DIR [--weights ...]`` prints the reference's summary
lines.  Where the reference copies every prediction to the host and synchronises after every forward (and, for stereo and depth,
once more per sample to skip empty masks), nothing here waits for the GPU until the result is asked for.
"""
import argparse
import glob
import os

import numpy as np
import torch

from .io import InputPadder, read_flo, read_kitti_disp, read_kitti_flow
from .metrics import DepthMetrics, FlowMetrics, StereoMetrics
from .prepost import geometry_for, image_size

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


def _grouped(samples, batch_size):
    """Consecutive samples whose images have one shape and dtype, up to ``batch_size`` at a time, as lists of stacked columns."""
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1')
    group = []
    for sample in samples:
        sample = tuple(torch.as_tensor(c) for c in sample)
        if group and (len(group) == batch_size or sample[0].shape != group[0][0].shape or sample[0].dtype != group[0][0].dtype):
            yield [torch.stack(c, 0) for c in zip(*group)]
            group = []
        group.append(sample)
    if group:
        yield [torch.stack(c, 0) for c in zip(*group)]


def _sized_prediction(model, geom, img0, img1, kind, forward_kw):
    """prepare -> forward -> ``(prediction, padder)`` for a metrics accumulator: a padded prediction stays padded and is read in
    place through the geometry's crop, a resized one is resized back (and rescaled) first."""
    img0, img1 = geom.prepare(img0, img1, normalize=img0.dtype == torch.uint8)
    with torch.no_grad():
        pred = model(img0, img1, **forward_kw)['flow_preds'][-1]
    if geom.mode == 'pad' and not geom.transpose:
        return pred, geom
    return geom.restore(pred, kind), None


def validate_stereo(model, samples, prefix, inference_size=None, padding_factor=32, max_disp=0., batch_size=1, **forward_kw):
    """``validate_things`` / ``validate_kitti15`` (evaluate_stereo.py:301-512) over ``samples``, an iterable of ``(left, right,
    disp_gt)``: images fp32 ``[3, H, W]`` as the reference's loader normalises them, or uint8 ``[H, W, 3]`` frames, which are
    normalised on the device; ``disp_gt [H, W]``.  Without ``inference_size`` the pair is padded as ``InputPadder(padding_factor=...)``
    pads it, else resized and the disparity resized back and scaled by ``W / wp``.  Pixels with ``disp_gt > 0`` count (and ``<
    max_disp`` when ``max_disp > 0``, as validate_things); a sample without one is skipped, as in the reference, but without asking
    the device per sample.  Returns ``<prefix>_epe``, ``_d1`` and ``_3px``: means of the per-sample values."""
    forward_kw = dict(forward_kw)
    forward_kw['task'] = 'stereo'
    metrics = StereoMetrics(max_disp)
    for left, right, disp_gt in (cols[:3] for cols in _grouped(samples, batch_size)):
        device = _model_device(model, left.device)
        left, right, disp_gt = (c.to(device, non_blocking=True) for c in (left, right, disp_gt))
        geom = geometry_for(image_size(left), inference_size, padding_factor, 'sintel')
        pred, padder = _sized_prediction(model, geom, left, right, 'disparity', forward_kw)
        metrics.update(pred, disp_gt.float(), padder)
    res = metrics.compute()
    return {f'{prefix}_{k}': res[name] for k, name in (('epe', 'epe'), ('d1', 'd1'), ('3px', 'thres3'))}


DEPTH_ERRORS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3')


def validate_depth(model, samples, prefix, inference_size=None, padding_factor=16, min_depth=0.5, max_depth=10., **forward_kw):
    """``validate_scannet`` (evaluate_depth.py:21-154) over ``samples``, an iterable of ``(img_ref, img_tgt, intrinsics, pose,
    depth_gt, valid)`` (images as in :func:`validate_stereo`, ``intrinsics [3, 3]``, ``pose [4, 4]``, ``depth_gt``, ``valid``
    ``[H, W]``).  Padding is ``InputPadder(mode='kitti')``'s; a resized prediction is resized back and NOT rescaled, and the
    intrinsics are left as they are, both as in the reference.  Pixels with ``min_depth < depth_gt < max_depth`` and ``valid > 0.5``
    count, and the model searches the inverse depths ``1 / max_depth .. 1 / min_depth`` (the reference's ``eval_*`` and model bounds
    have the same defaults; here they are one pair).  Returns ``<prefix>_abs_rel``
    ... ``_a3`` (the bare names for an empty prefix): means over the samples with a non-empty mask, as ``DepthMetrics`` skips the
    others (the reference skips them too but divides by the number of all samples)."""
    forward_kw = dict(forward_kw)
    forward_kw['task'] = 'depth'
    forward_kw.update(min_depth=1. / max_depth, max_depth=1. / min_depth)
    metrics = DepthMetrics(min_depth, max_depth)
    for cols in _grouped(samples, 1):
        device = _model_device(model, cols[0].device)
        img_ref, img_tgt, intrinsics, pose, depth_gt, valid = (c.to(device, non_blocking=True) for c in cols[:6])
        geom = geometry_for(image_size(img_ref), inference_size, padding_factor, 'kitti')
        kw = dict(forward_kw, intrinsics=intrinsics.float(), pose=pose.float())
        pred, padder = _sized_prediction(model, geom, img_ref, img_tgt, 'depth', kw)
        metrics.update(pred, depth_gt.float(), valid, padder)
    res = metrics.compute()
    return {(f'{prefix}_{k}' if prefix else k): res[k] for k in DEPTH_ERRORS}


def summary_lines(results, prefix, title):
    """The reference's ``print`` lines for one result dict."""
    r = {k[len(prefix) + 1:]: v for k, v in results.items() if k.startswith(prefix + '_')}
    lines = []
    if 'd1' in r:
        return ['Validation %s EPE: %.3f, D1: %.4f, 3px: %.4f' % (title, r['epe'], r['d1'], r['3px'])]
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


class Kitti15StereoPairs:
    """KITTI-2015 stereo, the layout of the reference's ``KITTI15`` dataset: ``training/image_2/*_10.png`` (left),
    ``training/image_3`` (right), ``training/disp_occ_0`` (16-bit disparity * 256) as ``(left, right, disp_gt)``.  The frames stay
    uint8 ``[H, W, 3]``: 3 bytes per pixel are uploaded and the ImageNet normalisation runs on the device."""

    def __init__(self, root):
        base = os.path.join(root, 'training')
        left = sorted(glob.glob(os.path.join(base, 'image_2', '*_10.png')))
        if not left:
            raise FileNotFoundError(os.path.join(base, 'image_2', '*_10.png'))
        self.items = [(p, p.replace('image_2', 'image_3'), p.replace('image_2', 'disp_occ_0')) for p in left]
        missing = [q for item in self.items for q in item[1:] if not os.path.exists(q)]
        if missing:
            raise FileNotFoundError(missing[0])

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        left, right, disp = self.items[index]
        from .video import read_frame_u8
        frames = [read_frame_u8(p) for p in (left, right)]
        return frames[0], frames[1], torch.from_numpy(read_kitti_disp(disp)[0])

    def __iter__(self):
        return (self[i] for i in range(len(self)))


# ------------------------------------------------------------------ command line
def build_parser():
    from .synth import CONFIGS
    ap = argparse.ArgumentParser(description="validation on the reference's Sintel / KITTI flow and KITTI-2015 stereo layouts, "
                                             'metrics on the device')
    ap.add_argument('--dataset', required=True, choices=MODES + ('kitti15-stereo',))
    ap.add_argument('--root', required=True, help='dataset directory (the one that holds training/)')
    ap.add_argument('--padding-factor', type=int, default=8, help="kitti15-stereo: the reference's script passes 32")
    ap.add_argument('--inference-size', type=int, nargs=2, default=None, metavar=('H', 'W'),
                    help='kitti15-stereo: resize to this size instead of padding')
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--with-speed-metric', action='store_true')
    ap.add_argument('--evaluate-matched-unmatched', action='store_true', help='Sintel only: reads training/occlusions')
    ap.add_argument('--per-sample', action='store_true', help="KITTI only: validate_kitti's average_over_pixels=False")
    ap.add_argument('--model-config', default='gmflow_s1',
                    choices=[k for k, v in CONFIGS.items() if v[1].get('task') in ('flow', 'stereo')],
                    help='a flow configuration for sintel / kitti, a stereo one for kitti15-stereo')
    ap.add_argument('--weights', default=None, help="checkpoint (the reference's: a state_dict, or {'model': state_dict}); "
                                                    'default: the seeded synthetic weights')
    ap.add_argument('--precision', default='exact', choices=['exact', 'fast'])
    return ap


def main(argv=None):
    from .model import UniMatch
    from .synth import CONFIGS, synth_state_dict
    args = build_parser().parse_args(argv)
    ck, fk = CONFIGS[args.model_config]
    task = 'stereo' if args.dataset == 'kitti15-stereo' else 'flow'
    if fk.get('task') != task:
        raise SystemExit(f'--dataset {args.dataset} needs a {task} configuration, {args.model_config} is for {fk.get("task")}')
    model = UniMatch(**ck).eval()
    if args.weights:
        sd = torch.load(args.weights, map_location='cpu')
        sd = sd.get('model', sd)
    else:
        sd = synth_state_dict({k: v.shape for k, v in model.state_dict().items()})
    model.load_state_dict(sd)
    model = model.to('cuda').set_precision(args.precision)
    fwd_kw = {k: v for k, v in fk.items() if k != 'task'}
    if task == 'stereo':
        pairs = Kitti15StereoPairs(args.root)
        print('=> %d samples found in the validation set' % len(pairs))
        results = validate_stereo(model, pairs, 'kitti15', inference_size=args.inference_size, padding_factor=args.padding_factor,
                                  batch_size=args.batch_size, **fwd_kw)
        print('\n'.join(summary_lines(results, 'kitti15', 'KITTI15')))
        return results
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
