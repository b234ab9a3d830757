"""Video post-processing and a frame-directory driver shaped like the reference's ``inference_flow`` (evaluate_flow.py:640-831).

  forward_backward_consistency_check(fwd, bwd, alpha, beta)   occlusion masks (unimatch/geometry.py:75-96)
  flow_to_image(flow)                                         Middlebury colouring (utils/flow_viz.py:231-254), per image

Both run on the HIP kernels (``um_fwd_bwd_occlusion``, ``um_flow_to_rgb``) for CUDA tensors.  For host tensors they run the host
restatement below, written step by step in the dtypes the reference evaluates them in (float32 up to the maximum radius, float64 from
the normalisation on, as NumPy 2 promotes); the CPU tests pin it against fixtures minted from the reference.

``python -m unimatch_amd.video --frames DIR --out DIR [...]`` runs :meth:`UniMatch.forward_sequence` over the ``*.png`` / ``*.jpg``
frames of a directory (sorted) and writes the reference's file set: ``%04d_flow.png``, ``%04d_flow_bwd.png``, ``%04d_occ_fwd.png`` /
``%04d_occ_bwd.png`` and ``%04d_pred.flo`` (``%04d_pred_bwd.flo``).  Reading frames needs PIL; video containers are not supported.
"""
import argparse
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

_UNKNOWN_FLOW = 1e7
# Middlebury colour wheel: six segments (RY, YG, GC, CB, BM, MR) of 15, 6, 4, 11, 13, 6 hues; a ramp of segment length n at step i
# is floor(255 i / n), rising into the segment's target channel or falling out of the previous one
_SEGMENTS = ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False))

_hip_ops = None


def _hip():
    global _hip_ops
    if _hip_ops is None:
        from .ops import HipOps            # raises when the HIP extension or the GPU is missing: there is no silent fallback
        _hip_ops = HipOps()
    return _hip_ops


def colour_wheel():
    """``[55, 3]`` float64, values 0..255."""
    rows = []
    for n, full, ramp, rising in _SEGMENTS:
        steps = np.floor(255 * np.arange(0, n) / n)
        seg = np.zeros((n, 3))
        seg[:, full] = 255
        seg[:, ramp] = steps if rising else 255 - steps
        rows.append(seg)
    return np.concatenate(rows, 0)


def _occlusion_host(fwd, bwd, alpha, beta):
    from .model import _warp
    mag = torch.norm(fwd, dim=1) + torch.norm(bwd, dim=1)
    diff_fwd = torch.norm(fwd + _warp(bwd, fwd), dim=1)
    diff_bwd = torch.norm(bwd + _warp(fwd, bwd), dim=1)
    thr = alpha * mag + beta
    return (diff_fwd > thr).float(), (diff_bwd > thr).float()


def forward_backward_consistency_check(fwd, bwd, alpha=0.01, beta=0.5):
    """``(occ_fwd, occ_bwd)`` ``[B, H, W]`` float in {0, 1} (1 = occluded) of the flows ``fwd``, ``bwd`` ``[B, 2, H, W]``: where the flow
    and the other direction's flow sampled at its target do not cancel, ``|fwd + bwd(p + fwd)| > alpha (|fwd| + |bwd|) + beta``."""
    if fwd.dim() != 4 or fwd.shape[1] != 2 or bwd.shape != fwd.shape:
        raise ValueError(f'expected two [B, 2, H, W] flows of one shape, got {tuple(fwd.shape)} and {tuple(bwd.shape)}')
    if fwd.is_cuda:
        with torch.cuda.device(fwd.device):
            return _hip().fwd_bwd_occlusion(fwd.float(), bwd.float(), alpha, beta)
    return _occlusion_host(fwd.float(), bwd.float(), alpha, beta)


def _flow_to_image_host(flow):
    """One ``[H, W, 2]`` float32 flow -> ``[H, W, 3]`` uint8."""
    u, v = flow[..., 0].astype(np.float32), flow[..., 1].astype(np.float32)        # copies: the caller's array is not written
    unknown = (np.abs(u) > _UNKNOWN_FLOW) | (np.abs(v) > _UNKNOWN_FLOW)
    u[unknown] = 0
    v[unknown] = 0
    rad32 = np.sqrt(u * u + v * v)                                                  # float32
    peak = np.max(rad32)
    maxrad = -1.0 if np.isnan(peak) else float(peak)                              # max(-1, NaN) is -1
    den = maxrad + np.finfo(np.float64).eps
    un, vn = u.astype(np.float64) / den, v.astype(np.float64) / den               # float64 from here on
    nan = np.isnan(un) | np.isnan(vn)
    un[nan] = 0
    vn[nan] = 0
    rad = np.sqrt(un * un + vn * vn)
    a = np.arctan2(-vn, -un) / np.pi
    fk = (a + 1) / 2 * 54 + 1
    k0 = np.floor(fk).astype(np.int64)
    k1 = k0 + 1
    k1[k1 == 56] = 1
    f = (fk - k0)[..., None]
    wheel = colour_wheel()
    col = (1 - f) * (wheel[k0 - 1] / 255) + f * (wheel[k1 - 1] / 255)
    inside = (rad <= 1)[..., None]
    col = np.where(inside, 1 - rad[..., None] * (1 - col), col * 0.75)
    img = np.floor(255 * col * (1 - nan.astype(np.int64))[..., None])
    img[unknown] = 0
    return img.astype(np.uint8)


def flow_to_image(flow):
    """Middlebury colouring of ``flow`` ``[B, 2, H, W]`` -> ``[B, H, W, 3]`` uint8, or ``[H, W, 2]`` -> ``[H, W, 3]`` (tensor or
    ndarray).  Each image is normalised by its own maximum radius; unknown flow (``|u|`` or ``|v| > 1e7``) is black."""
    hw2 = flow.dim() == 3 if torch.is_tensor(flow) else np.ndim(flow) == 3
    t = torch.as_tensor(flow)
    if hw2:
        if t.shape[-1] != 2:
            raise ValueError(f'expected [H, W, 2], got {tuple(t.shape)}')
        t = t.permute(2, 0, 1)[None]
    elif t.dim() != 4 or t.shape[1] != 2:
        raise ValueError(f'expected [B, 2, H, W] or [H, W, 2], got {tuple(t.shape)}')
    if t.is_cuda:
        with torch.cuda.device(t.device):
            out = _hip().flow_to_rgb(t.float())
    else:
        arr = t.float().permute(0, 2, 3, 1).numpy()
        out = torch.from_numpy(np.stack([_flow_to_image_host(a) for a in arr], 0))
    if hw2:
        out = out[0]
    return out if torch.is_tensor(flow) else out.cpu().numpy()


# ------------------------------------------------------------------ frame-directory driver
def list_frames(directory):
    return sorted(glob.glob(os.path.join(directory, '*.png')) + glob.glob(os.path.join(directory, '*.jpg')))


def _decode_rgb(path):
    try:
        from PIL import Image
    except ImportError as exc:  # pragma: no cover - depends on the host
        raise RuntimeError('reading frames needs PIL (python -c "import PIL" fails here)') from exc
    img = np.array(Image.open(path)).astype(np.uint8)
    return np.tile(img[..., None], (1, 1, 3)) if img.ndim == 2 else img[..., :3]


def read_frame(path):
    return torch.from_numpy(_decode_rgb(path)).permute(2, 0, 1).float()


def read_frame_u8(path):
    """The frame as the decoder delivers it: ``[H, W, 3]`` uint8 (the values of :func:`read_frame`, a quarter of the bytes)."""
    return torch.from_numpy(np.ascontiguousarray(_decode_rgb(path)))


def run_directory(model, paths, out_dir, fwd_kw, padding_factor=8, inference_size=None, pred_bidir_flow=False, fwd_bwd_check=False,
                  save_flo=False, pairs_per_launch=8, device='cuda', device_resize=False):
    """``inference_flow`` over the frames ``paths`` with the sequence mode: returns the number of pairs written.  ``device_resize``:
    upload the frames as uint8 and transpose / resize / resize back through :class:`unimatch_amd.prepost.InferenceGeometry` (one
    launch per step) instead of an fp32 upload and torch ops; the files written have the same names and the same format."""
    from .io import write_flo, write_png8
    from .prepost import InferenceGeometry
    if fwd_bwd_check and not pred_bidir_flow:
        raise ValueError('--fwd-bwd-check needs --pred-bidir-flow (as the reference asserts)')
    os.makedirs(out_dir, exist_ok=True)
    carry, pair = None, 0
    step = max(1, int(pairs_per_launch))
    i = 0
    while i < len(paths) - (1 if carry is None else 0):
        take = paths[i:i + step + (1 if carry is None else 0)]
        i += len(take)
        geom = None
        if device_resize:
            frames = torch.stack([read_frame_u8(p) for p in take], 0).to(device)
            geom = (InferenceGeometry.resized(frames.shape[1:3], inference_size, transpose='auto') if inference_size else
                    InferenceGeometry.nearest(frames.shape[1:3], padding_factor, transpose='auto'))
            frames, = geom.prepare(frames)
            transpose, size, ori = False, None, None                    # the geometry has done, and will undo, all of it
        else:
            frames = torch.stack([read_frame(p) for p in take], 0).to(device)
            transpose = frames.shape[-2] > frames.shape[-1]             # the model is trained with width > height
            if transpose:
                frames = frames.transpose(-2, -1)
            ori = tuple(frames.shape[-2:])
            size = tuple(inference_size) if inference_size else tuple(int(np.ceil(s / padding_factor)) * padding_factor for s in ori)
            if size != ori:
                frames = F.interpolate(frames, size=size, mode='bilinear', align_corners=True)
        out = model.forward_sequence(frames, pred_bidir_flow=pred_bidir_flow, pairs_per_launch=step, carry=carry, **fwd_kw)
        carry = out['carry']
        flows = [out['flow']] + ([out['flow_bwd']] if pred_bidir_flow else [])
        if geom is not None:
            flows = [geom.restore(f, 'flow') for f in flows]
        elif size != ori:                                               # back to the frame size, per-component scaling
            flows = [F.interpolate(f, size=ori, mode='bilinear', align_corners=True) for f in flows]
            for f in flows:
                f[:, 0] = f[:, 0] * ori[-1] / size[-1]
                f[:, 1] = f[:, 1] * ori[-2] / size[-2]
        if transpose:
            flows = [f.transpose(-2, -1) for f in flows]
        rgbs = [flow_to_image(f.contiguous()).cpu().numpy() for f in flows]
        occ = forward_backward_consistency_check(flows[0].contiguous(), flows[1].contiguous()) if fwd_bwd_check else None
        host = [f.permute(0, 2, 3, 1).cpu().numpy() for f in flows]
        for j in range(host[0].shape[0]):
            name = os.path.join(out_dir, '%04d' % (pair + j))
            write_png8(name + '_flow.png', rgbs[0][j])
            if pred_bidir_flow:
                write_png8(name + '_flow_bwd.png', rgbs[1][j])
            if occ is not None:
                write_png8(name + '_occ_fwd.png', (occ[0][j].cpu().numpy() * 255.).astype(np.uint8))
                write_png8(name + '_occ_bwd.png', (occ[1][j].cpu().numpy() * 255.).astype(np.uint8))
            if save_flo:
                write_flo(name + '_pred.flo', host[0][j])
                if pred_bidir_flow:
                    write_flo(name + '_pred_bwd.flo', host[1][j])
        pair += host[0].shape[0]
    return pair


def main(argv=None):
    from .model import UniMatch
    from .synth import CONFIGS, synth_state_dict
    ap = argparse.ArgumentParser(description='optical flow of a frame directory, every frame encoded once (UniMatch.forward_sequence)')
    ap.add_argument('--frames', required=True, help='directory of *.png / *.jpg frames, taken in sorted order')
    ap.add_argument('--out', required=True)
    ap.add_argument('--inference-size', type=int, nargs=2, default=None, metavar=('H', 'W'))
    ap.add_argument('--padding-factor', type=int, default=8)
    ap.add_argument('--pred-bidir-flow', action='store_true')
    ap.add_argument('--fwd-bwd-check', action='store_true')
    ap.add_argument('--save-flo', action='store_true')
    ap.add_argument('--model-config', default='gmflow_s1', choices=[k for k, v in CONFIGS.items() if v[1].get('task') == 'flow'])
    ap.add_argument('--weights', default=None, help="checkpoint (the reference's: a state_dict, or {'model': state_dict}); "
                                                    'default: the seeded synthetic weights')
    ap.add_argument('--precision', default='exact', choices=['exact', 'fast'])
    ap.add_argument('--pairs-per-launch', type=int, default=8)
    ap.add_argument('--device-resize', action='store_true', help='upload uint8 frames; transpose, resize and resize back on the device')
    args = ap.parse_args(argv)
    paths = list_frames(args.frames)
    print(f'{len(paths)} images found')
    if len(paths) < 2:
        raise SystemExit('need at least two frames')
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
    n = run_directory(model, paths, args.out, fwd_kw, padding_factor=args.padding_factor, inference_size=args.inference_size,
                      pred_bidir_flow=args.pred_bidir_flow, fwd_bwd_check=args.fwd_bwd_check, save_flo=args.save_flo,
                      pairs_per_launch=args.pairs_per_launch, device_resize=args.device_resize)
    print(f'{n} pairs written to {args.out}')


if __name__ == '__main__':
    main()
