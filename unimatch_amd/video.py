"""Video post-processing and a frame-directory driver shaped like the reference's ``inference_flow`` (evaluate_flow.py:640-831).

  forward_backward_consistency_check(fwd, bwd, alpha, beta)   occlusion masks (unimatch/geometry.py:75-96)
  flow_to_image(flow)                                         Middlebury colouring (utils/flow_viz.py:231-254), per image
  chain_flows(flow, occ, points, alive, stride)               long-range point tracks through the flows of consecutive pairs

They run on the HIP kernels (``um_fwd_bwd_occlusion``, ``um_flow_to_rgb``, ``um_flow_chain``) for CUDA tensors.  For host tensors they run the host
restatement below, written step by step in the dtypes the reference evaluates them in (float32 up to the maximum radius, float64 from
the normalisation on, as NumPy 2 promotes); the CPU tests pin it against fixtures minted from the reference.

``python -m unimatch_amd.video --frames DIR --out DIR [...]`` runs :meth:`UniMatch.forward_sequence` over the ``*.png`` / ``*.jpg``
frames of a directory (sorted) and writes the reference's file set: ``%04d_flow.png``, ``%04d_flow_bwd.png``, ``%04d_occ_fwd.png`` /
``%04d_occ_bwd.png`` and ``%04d_pred.flo`` (``%04d_pred_bwd.flo``); ``--track-grid S`` adds ``tracks.npz``, the tracks of every S-th
pixel of the first frame through the whole directory; ``--interpolate K`` adds ``%04d_tNNN.png``, K in-between frames of every pair
(:func:`interp.interpolate_frames`: a classical, unlearned synthesis), and ``--save-warped`` ``%04d_warped.png``, the pair's second
frame warped back onto the first by the forward flow.  Reading frames needs PIL; video containers are not supported.
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


# ------------------------------------------------------------------ point tracks
def start_grid(h, w, stride=1, device=None):
    """``[N, 2]`` float32 (x, y) of every ``stride``-th pixel of every ``stride``-th row, row-major: the start of ``points=None``."""
    ys, xs = torch.meshgrid(torch.arange(0, h, stride, device=device), torch.arange(0, w, stride, device=device), indexing='ij')
    return torch.stack([xs.reshape(-1), ys.reshape(-1)], -1).float()


def _chain_sample(planes, x, y):
    """Bilinear sample of ``planes [C, H, W]`` at the pixel positions (x, y) ``[N]``: taps outside the frame add zero.  Weights, tap
    order and the clamp before the integer conversion are those of ``chain_sample`` in csrc/video.hip."""
    c, h, w = planes.shape
    flat = planes.reshape(c, h * w)
    fx0, fy0 = torch.floor(x), torch.floor(y)
    fx1, fy1 = fx0 + 1.0, fy0 + 1.0
    wts = ((fx1 - x) * (fy1 - y), (x - fx0) * (fy1 - y), (fx1 - x) * (y - fy0), (x - fx0) * (y - fy0))
    x0 = torch.where(fx0 == fx0, fx0, torch.full_like(fx0, -2.0)).clamp(-2.0, w + 1.0).long()       # a NaN is outside
    y0 = torch.where(fy0 == fy0, fy0, torch.full_like(fy0, -2.0)).clamp(-2.0, h + 1.0).long()
    acc = torch.zeros(c, x.numel(), dtype=planes.dtype)
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        q = torch.where(inside, yy * w + xx, torch.zeros_like(yy))
        acc = torch.where(inside, acc + flat[:, q] * wt, acc)
    return acc


def _chain_flows_host(flow, occ, points, alive):
    """float32 restatement of ``um_flow_chain``: the documented step, one torch op per operation of the kernel."""
    p, _, h, w = flow.shape
    x, y = points[:, 0].clone(), points[:, 1].clone()

    def inside(x, y):
        return (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    alive = alive & inside(x, y)
    tracks, visible = [], []
    for t in range(p):
        uv = _chain_sample(flow[t], x, y)
        nx, ny = torch.where(alive, x + uv[0], x), torch.where(alive, y + uv[1], y)
        still = alive & inside(nx, ny)
        if occ is not None:
            still = still & ~(_chain_sample(occ[t][None], x, y)[0] >= 0.5)                     # the mask at the OLD position
        x, y, alive = nx, ny, still
        tracks.append(torch.stack([x, y], -1))
        visible.append(alive)
    return torch.stack(tracks, 0), torch.stack(visible, 0)


def chain_flows(flow, occ=None, points=None, alive=None, stride=1):
    """Follow points through the flows ``flow [P, 2, H, W]`` of ``P`` consecutive frame pairs (pair t maps frame t to frame t + 1)
    -> ``(tracks [P, N, 2] float32, visible [P, N] bool)``: ``tracks[t]`` are the (x, y) pixel positions in frame t + 1.

    ``points [N, 2]`` as (x, y) in the first frame; ``None`` is the grid of every ``stride``-th pixel of every ``stride``-th row
    (:func:`start_grid`; ``stride=1``: ``tracks[t] - grid`` is the dense long-range flow from frame 0 to frame t + 1, the composition
    ``F(0->t+1) = F(0->t) + flow_warp(F(t->t+1), F(0->t))`` of the reference's ``flow_warp``).  ``alive [N]`` bool: tracks to follow
    (``None``: all).  A point is inside when ``0 <= x <= W - 1`` and ``0 <= y <= H - 1``; a track starts alive when it is inside.  Each
    step adds the flow sampled bilinearly at the track (pixel coordinates, zeros outside) and the track stays alive while the new
    position is inside and, with ``occ [P, H, W]`` (1 = occluded, the ``occ_fwd`` of :func:`forward_backward_consistency_check`), the
    mask sampled at the OLD position is below 0.5.  A lost track keeps its last position and never recovers.  To continue a sequence
    pass ``points=tracks[-1], alive=visible[-1]``.  CUDA tensors run ``um_flow_chain`` (one launch), host tensors the float32
    restatement."""
    if not torch.is_tensor(flow) or flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] < 1:
        raise ValueError(f'flow: expected a [P, 2, H, W] tensor with P >= 1, got {tuple(getattr(flow, "shape", ()))}')
    if not flow.is_floating_point():
        raise ValueError(f'flow: expected a floating-point tensor, got {flow.dtype}')
    p, _, h, w = flow.shape
    if h < 2 or w < 2:
        raise ValueError(f'flow: H and W must be >= 2, got {h} x {w}')
    if occ is not None:
        if not torch.is_tensor(occ) or tuple(occ.shape) != (p, h, w):
            raise ValueError(f'occ: expected {(p, h, w)} (one mask per flow), got {tuple(getattr(occ, "shape", ()))}')
        if not occ.is_floating_point():
            raise ValueError(f'occ: expected a floating-point mask (1 = occluded), got {occ.dtype}')
        if occ.device != flow.device:
            raise ValueError(f'occ: on {occ.device}, flow is on {flow.device}')
    if points is not None:
        if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
            raise ValueError(f'points: expected [N, 2] as (x, y) with N >= 1, got {tuple(getattr(points, "shape", ()))}')
        if not points.is_floating_point():
            raise ValueError(f'points: expected a floating-point tensor, got {points.dtype}')
        if points.device != flow.device:
            raise ValueError(f'points: on {points.device}, flow is on {flow.device}')
        n = points.shape[0]
    else:
        if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
            raise ValueError(f'stride: expected an int >= 1, got {stride!r}')
        n = -(-h // stride) * -(-w // stride)
    if alive is not None:
        if not torch.is_tensor(alive) or alive.dtype != torch.bool or tuple(alive.shape) != (n,):
            raise ValueError(f'alive: expected a bool tensor of shape {(n,)}, got {tuple(getattr(alive, "shape", ()))} '
                             f'{getattr(alive, "dtype", type(alive))}')
        if alive.device != flow.device:
            raise ValueError(f'alive: on {alive.device}, flow is on {flow.device}')
    flow = flow.float()
    occ = None if occ is None else occ.float()
    points = None if points is None else points.float()
    if flow.is_cuda:
        with torch.cuda.device(flow.device):
            return _hip().flow_chain(flow, occ, points, alive, stride)
    if points is None:
        points = start_grid(h, w, stride)
    if alive is None:
        alive = torch.ones(n, dtype=torch.bool)
    return _chain_flows_host(flow, occ, points, alive)


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
                  save_flo=False, pairs_per_launch=8, device='cuda', device_resize=False, track_grid=0, save_confidence=False,
                  interpolate=0, save_warped=False):
    """``inference_flow`` over the frames ``paths`` with the sequence mode: returns the number of pairs written.  ``device_resize``:
    upload the frames as uint8 and transpose / resize / resize back through :class:`unimatch_amd.prepost.InferenceGeometry` (one
    launch per step) instead of an fp32 upload and torch ops; the files written have the same names and the same format.
    ``track_grid`` S > 0: follow every S-th pixel of the first frame through the restored flows (:func:`chain_flows`, with the forward
    occlusion mask when ``pred_bidir_flow``) and write ``tracks.npz``: ``tracks [T-1, N, 2]``, ``visible [T-1, N]``, ``start [N, 2]``.
    ``save_confidence``: also write ``<stem>_conf.png``, the peak matching probability of every feature pixel
    (``forward_sequence(return_confidence=True)``: taken in the same forward) nearest-upsampled to the frame and coloured.
    ``interpolate`` K > 0 (needs ``pred_bidir_flow``): also write ``<stem>_tNNN.png``, the K frames at the times ``t = k / (K + 1)``
    between the pair's two frames, ``NNN = round(1000 t)`` (:func:`interp.interpolate_frames` on the restored, frame-size flows and
    their occlusion masks).  ``save_warped``: also write ``<stem>_warped.png``, the pair's second frame warped back by the forward
    flow with zeros padding (:func:`interp.backward_warp`): where the flow is right it looks like the first frame."""
    from .io import write_flo, write_png8
    from .prepost import InferenceGeometry
    if fwd_bwd_check and not pred_bidir_flow:
        raise ValueError('--fwd-bwd-check needs --pred-bidir-flow (as the reference asserts)')
    if interpolate and not pred_bidir_flow:
        raise ValueError('--interpolate needs --pred-bidir-flow (the flows of both directions)')
    if interpolate or save_warped:
        from . import interp
    last_raw = None                                                     # the previous chunk's last frame as it was read
    os.makedirs(out_dir, exist_ok=True)
    carry, pair = None, 0
    track, tracks, visible = None, [], []                               # (positions, alive) after the last pair; per-chunk rows
    step = max(1, int(pairs_per_launch))
    i = 0
    while i < len(paths) - (1 if carry is None else 0):
        take = paths[i:i + step + (1 if carry is None else 0)]
        i += len(take)
        geom = None
        if device_resize:
            frames = raw = torch.stack([read_frame_u8(p) for p in take], 0).to(device)
            geom = (InferenceGeometry.resized(frames.shape[1:3], inference_size, transpose='auto') if inference_size else
                    InferenceGeometry.nearest(frames.shape[1:3], padding_factor, transpose='auto'))
            frames, = geom.prepare(frames)
            transpose, size, ori = False, None, None                    # the geometry has done, and will undo, all of it
        else:
            frames = raw = torch.stack([read_frame(p) for p in take], 0).to(device)
            transpose = frames.shape[-2] > frames.shape[-1]             # the model is trained with width > height
            if transpose:
                frames = frames.transpose(-2, -1)
            ori = tuple(frames.shape[-2:])
            size = tuple(inference_size) if inference_size else tuple(int(np.ceil(s / padding_factor)) * padding_factor for s in ori)
            if size != ori:
                frames = F.interpolate(frames, size=size, mode='bilinear', align_corners=True)
        seq_kw = dict(fwd_kw, return_confidence=True) if save_confidence else fwd_kw
        out = model.forward_sequence(frames, pred_bidir_flow=pred_bidir_flow, pairs_per_launch=step, carry=carry, **seq_kw)
        carry = out['carry']
        conf_rgb = None
        if save_confidence:                                             # taken in the same forward, at the matching step
            from .confidence import confidence_to_image
            conf = out['match_confidence']['max_prob']
            if transpose or (geom is not None and geom.transpose):
                conf = conf.transpose(-2, -1)
            shape = geom.shape if geom is not None else (ori[::-1] if transpose else ori)
            conf_rgb = confidence_to_image(conf, shape).cpu().numpy()
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
        occ = None
        if fwd_bwd_check or ((track_grid or interpolate) and pred_bidir_flow):
            occ = forward_backward_consistency_check(flows[0].contiguous(), flows[1].contiguous())
        if track_grid:
            trk, vis = chain_flows(flows[0].contiguous(), None if occ is None else occ[0], *(track or (None, None)), stride=track_grid)
            track = (trk[-1], vis[-1])
            tracks.append(trk.cpu().numpy())
            visible.append(vis.cpu().numpy())
        between = warped = None
        if interpolate or save_warped:                                  # on the frames as they were read, in either upload layout
            seen = raw if last_raw is None else torch.cat([last_raw, raw], 0)
            last_raw = raw[raw.shape[0] - 1:]
            tall = transpose or (geom is not None and geom.transpose)
            u8 = seen.dtype == torch.uint8
            use, use_occ = [f.contiguous() for f in flows], occ
            if tall:            # the flow's channels are those of the transposed image (the restore leaves them so): work there
                seen = seen.transpose(1, 2) if u8 else seen.transpose(-2, -1)
                use = [f.transpose(-2, -1).contiguous() for f in flows]
                use_occ = forward_backward_consistency_check(*use) if interpolate else None
            first, second = seen[:-1].contiguous(), seen[1:].contiguous()
            if interpolate:
                times = interp.between_times(interpolate)
                between = interp.interpolate_frames(first, second, use[0], use[1], times, occ_fwd=use_occ[0], occ_bwd=use_occ[1])
                between = (between.transpose(2, 3) if tall else between).cpu().numpy()
            if save_warped:
                warped = interp.backward_warp(second, use[0])
                if not u8:                                              # fp32 upload: [P, 3, H, W] in 0..255
                    warped = warped.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
                warped = (warped.transpose(1, 2) if tall else warped).cpu().numpy()
        if not fwd_bwd_check:
            occ = None
        host = [f.permute(0, 2, 3, 1).cpu().numpy() for f in flows]
        for j in range(host[0].shape[0]):
            name = os.path.join(out_dir, '%04d' % (pair + j))
            write_png8(name + '_flow.png', rgbs[0][j])
            if pred_bidir_flow:
                write_png8(name + '_flow_bwd.png', rgbs[1][j])
            if occ is not None:
                write_png8(name + '_occ_fwd.png', (occ[0][j].cpu().numpy() * 255.).astype(np.uint8))
                write_png8(name + '_occ_bwd.png', (occ[1][j].cpu().numpy() * 255.).astype(np.uint8))
            if conf_rgb is not None:
                write_png8(name + '_conf.png', conf_rgb[j])
            if between is not None:
                for n, t in enumerate(times):
                    write_png8(name + '_t%03d.png' % round(1000 * t), np.ascontiguousarray(between[j, n]))
            if warped is not None:
                write_png8(name + '_warped.png', np.ascontiguousarray(warped[j]))
            if save_flo:
                write_flo(name + '_pred.flo', host[0][j])
                if pred_bidir_flow:
                    write_flo(name + '_pred_bwd.flo', host[1][j])
        pair += host[0].shape[0]
    if track_grid:
        h, w = host[0].shape[1:3]
        np.savez(os.path.join(out_dir, 'tracks.npz'), tracks=np.concatenate(tracks, 0), visible=np.concatenate(visible, 0),
                 start=start_grid(h, w, track_grid).numpy())
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
    ap.add_argument('--track-grid', type=int, default=0, metavar='S',
                    help='follow every S-th pixel of the first frame through the sequence and write tracks.npz (0: off); with '
                         '--pred-bidir-flow a track also ends where the forward occlusion mask covers it')
    ap.add_argument('--save-confidence', action='store_true',
                    help='write <stem>_conf.png: the peak matching probability of every feature pixel, nearest-upsampled to the frame')
    ap.add_argument('--interpolate', type=int, default=0, metavar='K',
                    help='write <stem>_tNNN.png: K in-between frames of every pair at the times k / (K + 1), NNN = round(1000 t); a '
                         'classical synthesis from the two flows (no learned part), needs --pred-bidir-flow')
    ap.add_argument('--save-warped', action='store_true',
                    help='write <stem>_warped.png: the next frame warped back by the forward flow (zeros outside the frame)')
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
                      pairs_per_launch=args.pairs_per_launch, device_resize=args.device_resize, track_grid=args.track_grid,
                      save_confidence=args.save_confidence, interpolate=args.interpolate, save_warped=args.save_warped)
    print(f'{n} pairs written to {args.out}')


if __name__ == '__main__':
    main()
