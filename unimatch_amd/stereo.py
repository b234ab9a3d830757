"""A stereo-pair directory driver shaped like the reference's ``inference_stereo`` (evaluate_stereo.py:711-843).

``python -m unimatch_amd.stereo --dir DIR --out DIR [...]`` (the sorted ``*.png`` / ``*.jpg`` files alternate left, right) or
``--left DIR --right DIR`` runs :meth:`UniMatch.predict` over the pairs and writes, per pair, ``<stem>_disp.png`` (the reference's
``vis_disparity`` colouring, :mod:`unimatch_amd.visualize`), with ``--pred-bidir-disp`` also ``<stem>_disp_right.png`` (the right
view's disparity, mirrored back), and with ``--save-pfm-disp`` the disparities themselves as ``.pfm`` beside them.  Frames are uploaded
as uint8 and normalised on the device; like the reference's runner this one RESIZES -- to the next multiple of ``padding_factor`` or
to ``inference_size`` -- and never pads.  Resize, mirror, resize back, rescale and colouring are HIP launches; what crosses the bus per
pair is two uint8 frames up and one uint8 image (plus the fp32 disparity with ``--save-pfm-disp``) down.  Reading frames needs PIL.
"""
import argparse
import os

import numpy as np
import torch

from .video import list_frames, read_frame_u8
from .visualize import disparity_to_image


def nearest_size(shape, padding_factor):
    """The reference's default inference size: each dimension rounded up to a multiple of ``padding_factor``."""
    return tuple(int(np.ceil(s / padding_factor)) * padding_factor for s in shape)


def run_stereo(model, left_paths, right_paths, out_dir, fwd_kw, padding_factor=16, inference_size=None, pred_bidir_disp=False,
               pred_right_disp=False, save_pfm_disp=False, batch_size=1, device='cuda', lr_check=False):
    """``inference_stereo`` over the pairs ``(left_paths[i], right_paths[i])``: returns the number of pairs written.  Consecutive
    pairs of one size are predicted ``batch_size`` at a time.  ``lr_check``: also the left / right occlusion masks."""
    from .geometry import disparity_consistency_check
    from .io import write_pfm, write_png8
    if len(left_paths) != len(right_paths):
        raise ValueError(f'{len(left_paths)} left and {len(right_paths)} right images')
    if lr_check and not pred_bidir_disp:
        raise ValueError('--lr-check needs --pred-bidir-disp (both views are compared)')
    os.makedirs(out_dir, exist_ok=True)
    fwd_kw = {k: v for k, v in fwd_kw.items() if k != 'task'}
    step = max(1, int(batch_size))
    done = 0
    while done < len(left_paths):
        lefts, rights = [read_frame_u8(left_paths[done])], [read_frame_u8(right_paths[done])]
        while len(lefts) < step and done + len(lefts) < len(left_paths):
            nxt = read_frame_u8(left_paths[done + len(lefts)])
            if nxt.shape != lefts[0].shape:
                break
            lefts.append(nxt)
            rights.append(read_frame_u8(right_paths[done + len(rights)]))
        n = len(lefts)
        left, right = torch.stack(lefts, 0).to(device), torch.stack(rights, 0).to(device)
        size = tuple(inference_size) if inference_size else nearest_size(left.shape[1:3], padding_factor)
        with torch.no_grad():
            disp = model.predict(left, right, inference_size=size, pred_right_disp=pred_right_disp, pred_bidir_disp=pred_bidir_disp,
                                 task='stereo', **fwd_kw)['flow_preds'][-1]                  # [n or 2n, H, W]
        rgb = disparity_to_image(disp).cpu().numpy()
        host = disp.cpu().numpy() if save_pfm_disp else None
        occ = None
        if lr_check:
            occ = [(o.cpu().numpy() * 255.).astype(np.uint8) for o in disparity_consistency_check(disp[:n].contiguous(), disp[n:].contiguous())]
        for j in range(n):
            stem = os.path.join(out_dir, os.path.splitext(os.path.basename(left_paths[done + j]))[0])
            outputs = [('_disp', j)] + ([('_disp_right', n + j)] if pred_bidir_disp else [])
            for suffix, row in outputs:
                write_png8(stem + suffix + '.png', rgb[row])
                if save_pfm_disp:
                    write_pfm(stem + suffix + '.pfm', host[row])
            if occ is not None:
                write_png8(stem + '_occ.png', occ[0][j])
                write_png8(stem + '_occ_right.png', occ[1][j])
        done += n
    return done


def pair_lists(directory=None, left_dir=None, right_dir=None):
    """``(left_paths, right_paths)`` as the reference lists them: one directory whose sorted files alternate, or two directories."""
    if directory:
        names = list_frames(directory)
        return names[::2], names[1::2]
    if not (left_dir and right_dir):
        raise ValueError('give --dir, or --left and --right')
    return list_frames(left_dir), list_frames(right_dir)


def load_model(model_config, weights, precision, device='cuda'):
    """The model of a ``synth.CONFIGS`` entry with a checkpoint (the reference's: a state_dict, or ``{'model': state_dict}``) or the
    seeded synthetic weights, and the entry's forward keywords."""
    from .model import UniMatch
    from .synth import CONFIGS, synth_state_dict
    ck, fk = CONFIGS[model_config]
    model = UniMatch(**ck).eval()
    if weights:
        sd = torch.load(weights, map_location='cpu')
        sd = sd.get('model', sd)
    else:
        sd = synth_state_dict({k: v.shape for k, v in model.state_dict().items()})
    model.load_state_dict(sd)
    return model.to(device).set_precision(precision), dict(fk)


def main(argv=None):
    from .synth import CONFIGS
    ap = argparse.ArgumentParser(description='disparity of a directory of stereo pairs (UniMatch.predict), coloured on the device')
    ap.add_argument('--dir', default=None, help='one directory: the sorted *.png / *.jpg files alternate left, right')
    ap.add_argument('--left', default=None, help='directory of left images (with --right)')
    ap.add_argument('--right', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--inference-size', type=int, nargs=2, default=None, metavar=('H', 'W'))
    ap.add_argument('--padding-factor', type=int, default=16)
    ap.add_argument('--pred-bidir-disp', action='store_true')
    ap.add_argument('--pred-right-disp', action='store_true')
    ap.add_argument('--save-pfm-disp', action='store_true')
    ap.add_argument('--lr-check', action='store_true', help='with --pred-bidir-disp: write the left / right occlusion masks (0 / 255)')
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--model-config', default='gmstereo_s1', choices=[k for k, v in CONFIGS.items() if v[1].get('task') == 'stereo'])
    ap.add_argument('--weights', default=None, help="checkpoint (the reference's: a state_dict, or {'model': state_dict}); "
                                                    'default: the seeded synthetic weights')
    ap.add_argument('--precision', default='exact', choices=['exact', 'fast'])
    args = ap.parse_args(argv)
    lefts, rights = pair_lists(args.dir, args.left, args.right)
    print(f'{len(lefts)} test samples found')
    if not lefts or len(lefts) != len(rights):
        raise SystemExit(f'need as many left as right images, got {len(lefts)} and {len(rights)}')
    model, fwd_kw = load_model(args.model_config, args.weights, args.precision)
    n = run_stereo(model, lefts, rights, args.out, fwd_kw, padding_factor=args.padding_factor, inference_size=args.inference_size,
                   pred_bidir_disp=args.pred_bidir_disp, pred_right_disp=args.pred_right_disp, save_pfm_disp=args.save_pfm_disp,
                   batch_size=args.batch_size, lr_check=args.lr_check)
    print(f'{n} pairs written to {args.out}')


if __name__ == '__main__':
    main()
