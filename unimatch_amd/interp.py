"""Frame synthesis from flow: warp an image by a flow, move a flow to an intermediate time, synthesise in-between frames.

This is a CLASSICAL synthesis with no learned refinement network: flow reversal by forward splatting, two backward warps and an
occlusion-aware blend.  It is exact where the flow is exact (a zero flow cross-fades, a constant translation reproduces the shifted
frame bit for bit) and makes no claim about quality on real flows.

  backward_warp(image, flow, padding='zeros', return_mask=False)   ``out(p) = bilinear(image, p + flow(p))``: the reference's
                                                                   ``flow_warp`` (unimatch/geometry.py:41-72) applied to an image
  splat_flow(flow, times, weight=None, min_weight=1/256)           the flow moved to each time t by forward splatting: every source
                                                                   pixel p adds its flow around ``p + t flow(p)``
  interpolate_frames(img0, img1, flow_fwd, flow_bwd, times, ...)   K in-between frames of every pair ``[B, K, H, W, 3]`` uint8

Images are ``[B, C, H, W]`` float32 (any C >= 1; values 0..255 and C = 3 for ``interpolate_frames``) or ``[B, H, W, 3]`` uint8, flows
``[B, 2, H, W]`` (x, y).  CUDA tensors run the kernels of ``csrc/interp.hip`` (``um_image_warp``, ``um_flow_splat``,
``um_frame_synthesize``); host tensors run the ``*_host`` restatement below, written operation by operation in the kernels' order and
precision (float32 without contraction, float64 and int64 where stated).  The two are bitwise equal, and there is no silent fallback
from one to the other.

``backward_warp``: the sample position goes through the reference's normalise / un-normalise round trip (``g = 2 p / (n - 1) - 1``,
``i = ((g + 1) / 2) (n - 1)``), as ``forward_backward_consistency_check`` does.  ``'zeros'``: taps outside the frame add nothing;
``'border'``: the position is clamped into the frame first (a NaN goes to 0).  A uint8 output is ``rint`` of the float32 sum, clamped to
0..255.  The mask is the reference's ``return_mask``: ``-1 <= g <= 1`` in x and y.

``splat_flow``: source pixel ``p = (x, y)`` with flow ``(u, v)`` lands at ``X = (float)x + t u``, ``Y = (float)y + t v``.  With
``ax = X - floor(X)`` its four taps are ``(1 - ax)(1 - ay)``, ``ax (1 - ay)``, ``(1 - ax) ay``, ``ax ay``, each multiplied by
``weight[b, y, x]`` (clamped to <= 1; NaN, infinite or <= 0: the pixel contributes nothing).  A pixel whose flow is not finite or
exceeds 32768 px in either component contributes nothing.  The sums are INTEGERS, so that they do not depend on the order of the
additions: ``wq = (int64) rint(wt 65536)``, ``uq = (int64) rint(256 u)``, and per (b, t) three int64 planes ``S_w += wq``,
``S_u += wq uq``, ``S_v += wq vq`` (``index_add_`` here, 64-bit integer atomic adds on the device).  The result is
``(float)((double)S_u / (double)S_w / 256.0)`` and ``hole = S_w < max(1, rint(min_weight 65536))``; the flow of a hole is 0.
``|S| <= H W 2^39``, so ``H W`` is capped at 2^21.

``interpolate_frames``, per output pixel q and time t (``t' = 1 - t`` in float32):

1. ``A`` = the forward flow splatted to t, ``B`` = the backward flow splatted to t'.  Both valid: ``m = 0.5 (A + (-B))``; one valid:
   that one (``A`` or ``-B``); neither: ``m = 0`` and q is a hole.
2. ``c0 = bilinear(img0, q - t m)``, ``c1 = bilinear(img1, q + t' m)`` with border clamping; ``v0``, ``v1`` are 1 iff the unclamped
   position lies in ``[0, W - 1] x [0, H - 1]``.
3. With masks (``[B, H, W]`` float, 1 = occluded, as ``forward_backward_consistency_check`` returns them): ``o0`` = ``occ_fwd`` sampled
   at ``q - t m``, ``o1`` = ``occ_bwd`` at ``q + t' m`` (bilinear, zeros outside); without masks both are 0.
4. ``w0 = t' v0 (1 - o1)``, ``w1 = t v1 (1 - o0)``: content of frame 0 that frame 1 no longer shows comes from frame 0, and the other
   way round.  If ``w0 + w1 < 1e-6``: ``w0 = t'``, ``w1 = t``.
5. ``out = rint((w0 c0 + w1 c1) / (w0 + w1))`` clamped to 0..255.

Every bilinear sample takes the taps NW, NE, SW, SE with the weights ``(x1 - x)(y1 - y)`` ... of ``occ_sample`` (csrc/video.hip) and adds
the in-frame ones in that order.
"""
import ctypes

import numpy as np
import torch

from . import _abi

MAX_TIMES = 16                   # UM_INTERP_MAX_TIMES
MAX_PIXELS = 1 << 21             # the cap on H W of the splat: |S| <= H W 2^39 stays below 2^63
MAX_FLOW = 32768.0
_F32, _U8 = 0, 1                 # UM_IMG_F32_NCHW, UM_IMG_U8_NHWC


# ------------------------------------------------------------------ argument checks
def _times32(times):
    """``times`` as a float32 array ``[K]``, 1 <= K <= 16, every value strictly between 0 and 1."""
    t = np.asarray([float(v) for v in times], dtype=np.float32)
    if t.ndim != 1 or not 1 <= t.size <= MAX_TIMES:
        raise ValueError(f'times: expected 1 to {MAX_TIMES} values, got {t.size}')
    if not bool(np.all((t > 0) & (t < 1))):
        raise ValueError(f'times: every value must lie strictly between 0 and 1, got {t.tolist()}')
    return t


def _hole_threshold(min_weight):
    """``max(1, rint(min_weight 65536))`` with the product in float32: a pixel that received nothing is always a hole."""
    mw = np.float32(min_weight)
    if not (mw >= 0 and mw <= 1):
        raise ValueError(f'min_weight: expected a value in [0, 1], got {min_weight!r}')
    return max(1, int(np.rint(mw * np.float32(65536.0))))


def _layout(image, name='image'):
    """``(layout, B, C, H, W)`` of an image tensor in one of the two layouts."""
    if not torch.is_tensor(image) or image.dim() != 4:
        raise ValueError(f'{name}: expected a [B, C, H, W] float32 or [B, H, W, 3] uint8 tensor, got {tuple(getattr(image, "shape", ()))}')
    if image.dtype == torch.uint8:
        if image.shape[3] != 3:
            raise ValueError(f'{name}: a uint8 image is [B, H, W, 3], got {tuple(image.shape)}')
        return _U8, image.shape[0], 3, image.shape[1], image.shape[2]
    if image.dtype != torch.float32:
        raise ValueError(f'{name}: expected float32 ([B, C, H, W]) or uint8 ([B, H, W, 3]), got {image.dtype}')
    if image.shape[1] < 1:
        raise ValueError(f'{name}: no channel')
    return (_F32,) + tuple(image.shape)


def _check_flow(flow, b, h, w, name='flow', device=None):
    if not torch.is_tensor(flow) or tuple(flow.shape) != (b, 2, h, w) or not flow.is_floating_point():
        raise ValueError(f'{name}: expected a floating-point {(b, 2, h, w)} tensor, got {tuple(getattr(flow, "shape", ()))} '
                         f'{getattr(flow, "dtype", type(flow))}')
    if device is not None and flow.device != device:
        raise ValueError(f'{name}: on {flow.device}, expected {device}')
    if h < 2 or w < 2:
        raise ValueError(f'{name}: H and W must be >= 2, got {h} x {w}')


def _check_plane(t, b, h, w, name, device):
    if t is None:
        return None
    if not torch.is_tensor(t) or tuple(t.shape) != (b, h, w) or not t.is_floating_point():
        raise ValueError(f'{name}: expected a floating-point {(b, h, w)} tensor, got {tuple(getattr(t, "shape", ()))}')
    if t.device != device:
        raise ValueError(f'{name}: on {t.device}, expected {device}')
    return t.float().contiguous()


def _check_splat_size(h, w):
    if h * w > MAX_PIXELS:
        raise ValueError(f'{h} x {w}: the splat accumulates in int64 and is limited to H W <= 2^21 pixels')


# ------------------------------------------------------------------ host restatement
def _planes(image, layout):
    """``[B, C, L]`` float32 planes of an image in either layout."""
    if layout == _U8:
        return image.permute(0, 3, 1, 2).reshape(image.shape[0], 3, -1).float()
    return image.reshape(image.shape[0], image.shape[1], -1)


def _taps_host(ix, iy, h, w):
    """``make_taps`` of csrc/interp.hip for positions ``[B, L]``: the four weights (NW, NE, SW, SE) and the clamped integer corner."""
    fx0, fy0 = torch.floor(ix), torch.floor(iy)
    fx1, fy1 = fx0 + 1.0, fy0 + 1.0
    wts = ((fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0))
    x0 = torch.where(fx0 == fx0, fx0, torch.full_like(fx0, -2.0)).clamp(-2.0, w + 1.0).long()       # a NaN is outside
    y0 = torch.where(fy0 == fy0, fy0, torch.full_like(fy0, -2.0)).clamp(-2.0, h + 1.0).long()
    return wts, x0, y0


def _gather_host(planes, taps, h, w):
    """Sum of the in-frame taps of ``planes [B, C, L]``, in the order NW, NE, SW, SE -> ``[B, C, L']``."""
    wts, x0, y0 = taps
    acc = torch.zeros(planes.shape[0], planes.shape[1], x0.shape[1], dtype=planes.dtype)
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
        yy, xx = y0 + dy, x0 + dx
        inside = ((yy >= 0) & (yy < h) & (xx >= 0) & (xx < w))[:, None]
        q = torch.where(inside[:, 0], yy * w + xx, torch.zeros_like(yy))
        v = torch.gather(planes, 2, q[:, None].expand(-1, planes.shape[1], -1))
        acc = torch.where(inside, acc + v * wt[:, None], acc)
    return acc


def _clamp_pos(p, n):
    return torch.where(p == p, p, torch.zeros_like(p)).clamp(0.0, float(n - 1))                      # a NaN goes to 0


def _pixel_xy(h, w):
    i = torch.arange(h * w)
    return (i % w).float()[None], (i // w).float()[None]


def _to_byte(v):
    return torch.where(v == v, torch.round(v), torch.zeros_like(v)).clamp(0.0, 255.0).to(torch.uint8)


def _image_out(planes, layout, b, c, h, w):
    if layout == _U8:
        return _to_byte(planes).view(b, 3, h, w).permute(0, 2, 3, 1).contiguous()
    return planes.view(b, c, h, w)


def backward_warp_host(image, flow, padding='zeros', return_mask=False):
    """``um_image_warp`` step by step in float32."""
    layout, b, c, h, w = _layout(image)
    f = flow.float().reshape(b, 2, h * w)
    x, y = _pixel_xy(h, w)
    px, py = x + f[:, 0], y + f[:, 1]
    gx, gy = 2.0 * px / float(w - 1) - 1.0, 2.0 * py / float(h - 1) - 1.0
    ix, iy = ((gx + 1.0) / 2.0) * float(w - 1), ((gy + 1.0) / 2.0) * float(h - 1)
    mask = ((gx >= -1.0) & (gy >= -1.0) & (gx <= 1.0) & (gy <= 1.0)).view(b, h, w)
    if padding == 'border':
        ix, iy = _clamp_pos(ix, w), _clamp_pos(iy, h)
    out = _image_out(_gather_host(_planes(image, layout), _taps_host(ix, iy, h, w), h, w), layout, b, c, h, w)
    return (out, mask) if return_mask else out


def splat_accumulate_host(flow, times, weight=None):
    """The accumulators of ``um_flow_splat`` for one direction: int64 ``[B, K, 3, H, W]`` (planes ``S_w``, ``S_u``, ``S_v``).
    ``times``: float32 values."""
    b, _, h, w = flow.shape
    L = h * w
    f = flow.float().reshape(b, 2, L)
    u, v = f[:, 0], f[:, 1]
    ok = (u.abs() <= MAX_FLOW) & (v.abs() <= MAX_FLOW)                                  # false for a NaN
    g = torch.ones(b, L)
    if weight is not None:
        g = weight.float().reshape(b, L)
        ok = ok & (g > 0) & (g != float('inf'))
        g = torch.where(ok, g, torch.ones_like(g)).clamp(max=1.0)
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    uq, vq = torch.round(u * 256.0).long(), torch.round(v * 256.0).long()
    x, y = _pixel_xy(h, w)
    image = (torch.arange(b) * L)[:, None]
    out = torch.zeros(b, len(times), 3, L, dtype=torch.int64)
    for kk, t in enumerate(times):
        t = torch.tensor(float(t), dtype=torch.float32)
        X, Y = x + t * u, y + t * v
        fx0, fy0 = torch.floor(X), torch.floor(Y)
        ax, ay = X - fx0, Y - fy0
        x0, y0 = fx0.long(), fy0.long()
        planes = [torch.zeros(b * L, dtype=torch.int64) for _ in range(3)]
        for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)),
                                ((1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay)):
            wq = torch.round((wt * g) * 65536.0).long()
            yy, xx = y0 + dy, x0 + dx
            hit = ok & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) & (wq > 0)
            wq = torch.where(hit, wq, torch.zeros_like(wq))
            q = (torch.where(hit, yy * w + xx, torch.zeros_like(yy)) + image).reshape(-1)
            for plane, val in zip(planes, (wq, wq * uq, wq * vq)):
                plane.index_add_(0, q, val.reshape(-1))
        out[:, kk] = torch.stack(planes, 0).view(3, b, L).transpose(0, 1)
    return out.view(b, len(times), 3, h, w)


def splat_normalize_host(acc, threshold):
    """``(flow [B, K, 2, H, W] float32, hole [B, K, H, W] bool)`` of the accumulators ``[B, K, 3, H, W]``: float64 quotients."""
    sw = acc[:, :, 0]
    hole = sw < threshold
    den = torch.where(hole, torch.ones_like(sw), sw).double()
    avg = torch.stack([(acc[:, :, 1].double() / den / 256.0).float(), (acc[:, :, 2].double() / den / 256.0).float()], 2)
    return torch.where(hole[:, :, None], torch.zeros_like(avg), avg), hole


def splat_flow_host(flow, times, weight=None, min_weight=1.0 / 256):
    return splat_normalize_host(splat_accumulate_host(flow, _times32(times), weight), _hole_threshold(min_weight))


def synthesize_host(img0, img1, acc_fwd, acc_bwd, times, occ_fwd=None, occ_bwd=None, min_weight=1.0 / 256):
    """``um_frame_synthesize`` step by step: ``(frames [B, K, H, W, 3] uint8, holes [B, K, H, W] bool)`` from the accumulators of the
    forward flow at ``times`` and of the backward flow at ``1 - times`` (float32)."""
    layout, b, c, h, w = _layout(img0, 'img0')
    thr = _hole_threshold(min_weight)
    p0, p1 = _planes(img0, layout), _planes(img1, layout)
    fa, hole_a = splat_normalize_host(acc_fwd, thr)
    fb, hole_b = splat_normalize_host(acc_bwd, thr)
    x, y = _pixel_xy(h, w)
    frames, holes = [], []
    for kk, t in enumerate(times):
        t, t1 = torch.tensor(float(t), dtype=torch.float32), torch.tensor(float(np.float32(1.0) - np.float32(t)), dtype=torch.float32)
        va, vb = ~hole_a[:, kk].reshape(b, -1), ~hole_b[:, kk].reshape(b, -1)
        a, bb = fa[:, kk].reshape(b, 2, -1), fb[:, kk].reshape(b, 2, -1)
        both = (va & vb)[:, None]
        m = torch.where(both, 0.5 * (a + (-bb)), torch.where(va[:, None], a, torch.where(vb[:, None], -bb, torch.zeros_like(a))))
        x0, y0 = x - t * m[:, 0], y - t * m[:, 1]
        x1, y1 = x + t1 * m[:, 0], y + t1 * m[:, 1]
        v0 = (x0 >= 0) & (x0 <= w - 1) & (y0 >= 0) & (y0 <= h - 1)
        v1 = (x1 >= 0) & (x1 <= w - 1) & (y1 >= 0) & (y1 <= h - 1)
        c0 = _gather_host(p0, _taps_host(_clamp_pos(x0, w), _clamp_pos(y0, h), h, w), h, w)
        c1 = _gather_host(p1, _taps_host(_clamp_pos(x1, w), _clamp_pos(y1, h), h, w), h, w)
        zero = torch.zeros(b, h * w)
        o0 = zero if occ_fwd is None else _gather_host(occ_fwd.float().reshape(b, 1, -1), _taps_host(x0, y0, h, w), h, w)[:, 0]
        o1 = zero if occ_bwd is None else _gather_host(occ_bwd.float().reshape(b, 1, -1), _taps_host(x1, y1, h, w), h, w)[:, 0]
        w0 = torch.where(v0, t1 * (1.0 - o1), zero)
        w1 = torch.where(v1, t * (1.0 - o0), zero)
        ws = w0 + w1
        plain = ~(ws >= 1e-6)
        w0, w1 = torch.where(plain, t1.expand_as(w0), w0), torch.where(plain, t.expand_as(w1), w1)
        ws = w0 + w1
        val = (w0[:, None] * c0 + w1[:, None] * c1) / ws[:, None]
        frames.append(_to_byte(val).view(b, 3, h, w).permute(0, 2, 3, 1))
        holes.append(~(va | vb).view(b, h, w))
    return torch.stack(frames, 1).contiguous(), torch.stack(holes, 1)


def interpolate_frames_host(img0, img1, flow_fwd, flow_bwd, times, occ_fwd=None, occ_bwd=None, min_weight=1.0 / 256):
    t = _times32(times)
    acc_f = splat_accumulate_host(flow_fwd, t, None)
    acc_b = splat_accumulate_host(flow_bwd, np.float32(1.0) - t, None)
    return synthesize_host(img0, img1, acc_f, acc_b, t, occ_fwd, occ_bwd, min_weight)


# ------------------------------------------------------------------ the library
def _ptr(t):
    return None if t is None else t.data_ptr()


def _host_times(rows):
    arr = np.ascontiguousarray(np.concatenate(rows).astype(np.float32))
    return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def splat_accumulators(flow_fwd, times_fwd, flow_bwd=None, times_bwd=None, weight_fwd=None, weight_bwd=None, min_weight=1.0 / 256,
                       normalize=False):
    """``um_flow_splat`` on CUDA flows: the int64 accumulators ``[dirs, B, K, 3, H, W]`` of one launch over one or two directions
    (they are the call's workspace) and, with ``normalize``, ``(flow [dirs, B, K, 2, H, W], hole [dirs, B, K, H, W] uint8)``."""
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    b, _, h, w = flow_fwd.shape
    dirs, k = (1 if flow_bwd is None else 2), len(times_fwd)
    tarr, tptr = _host_times([times_fwd] + ([] if flow_bwd is None else [times_bwd]))
    dev = flow_fwd.device
    with torch.cuda.device(dev):
        acc = torch.empty((dirs, b, k, 3, h, w), dtype=torch.int64, device=dev)
        avg = torch.empty((dirs, b, k, 2, h, w), dtype=torch.float32, device=dev) if normalize else None
        hole = torch.empty((dirs, b, k, h, w), dtype=torch.uint8, device=dev) if normalize else None
        _abi.check(lib.um_flow_splat(flow_fwd.data_ptr(), _ptr(flow_bwd), _ptr(weight_fwd), _ptr(weight_bwd), tptr, b, k, h, w,
                                     float(min_weight), _ptr(avg), _ptr(hole), acc.data_ptr(), acc.numel() * 8, _stream()),
                   'um_flow_splat')
    return acc, avg, hole


# ------------------------------------------------------------------ public functions
def backward_warp(image, flow, *, padding='zeros', return_mask=False):
    """``out(p) = bilinear(image, p + flow(p))`` in the layout and dtype of ``image`` (``[B, C, H, W]`` float32 or ``[B, H, W, 3]`` uint8);
    ``flow [B, 2, H, W]``.  ``padding``: ``'zeros'`` (the reference's ``flow_warp(image, flow)``) or ``'border'``.  ``return_mask``:
    also the reference's mask ``[B, H, W]`` bool, true where the sample position lies inside the frame."""
    if padding not in ('zeros', 'border'):
        raise ValueError(f"padding must be 'zeros' or 'border', got {padding!r}")
    layout, b, c, h, w = _layout(image)
    _check_flow(flow, b, h, w, device=image.device)
    if not image.is_cuda:
        return backward_warp_host(image, flow, padding, return_mask)
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    image, flow = image.contiguous(), flow.float().contiguous()
    with torch.cuda.device(image.device):
        out = torch.empty_like(image)
        mask = torch.empty((b, h, w), dtype=torch.uint8, device=image.device) if return_mask else None
        _abi.check(lib.um_image_warp(image.data_ptr(), layout, flow.data_ptr(), out.data_ptr(), _ptr(mask), b, c, h, w,
                                     int(padding == 'border'), _stream()), 'um_image_warp')
    return (out, mask.bool()) if return_mask else out


def splat_flow(flow, times, *, weight=None, min_weight=1.0 / 256):
    """Move ``flow [B, 2, H, W]`` to each time of ``times`` (up to 16 values in (0, 1)) by forward splatting ->
    ``(flow [B, K, 2, H, W] float32, hole [B, K, H, W] bool)``.  ``weight [B, H, W]``: a per-source-pixel confidence (clamped to <= 1;
    non-finite or <= 0 contributes nothing).  A pixel that received less than ``min_weight`` in total is a hole, with flow 0."""
    if not torch.is_tensor(flow) or flow.dim() != 4:
        raise ValueError(f'flow: expected a [B, 2, H, W] tensor, got {tuple(getattr(flow, "shape", ()))}')
    b, _, h, w = flow.shape
    _check_flow(flow, b, h, w)
    _check_splat_size(h, w)
    t = _times32(times)
    thr = _hole_threshold(min_weight)
    weight = _check_plane(weight, b, h, w, 'weight', flow.device)
    if not flow.is_cuda:
        return splat_normalize_host(splat_accumulate_host(flow, t, weight), thr)
    _, avg, hole = splat_accumulators(flow.float().contiguous(), t, weight_fwd=weight, min_weight=min_weight, normalize=True)
    return avg[0], hole[0].bool()


def interpolate_frames(img0, img1, flow_fwd, flow_bwd, times, *, occ_fwd=None, occ_bwd=None, return_holes=False,
                       min_weight=1.0 / 256):
    """``[B, K, H, W, 3]`` uint8: the frames at the ``times`` (in (0, 1)) between ``img0`` and ``img1`` (``[B, 3, H, W]`` float32 in
    0..255, or ``[B, H, W, 3]`` uint8) from the flows ``img0 -> img1`` and ``img1 -> img0``; the steps are in the module's docstring.
    ``occ_fwd``, ``occ_bwd`` ``[B, H, W]`` float (1 = occluded): the masks of ``forward_backward_consistency_check``.
    ``return_holes``: also ``[B, K, H, W]`` bool, true where neither splat reached the pixel.  On the device: two launches."""
    layout, b, c, h, w = _layout(img0, 'img0')
    if c != 3:
        raise ValueError(f'img0: expected 3 channels, got {c}')
    if not torch.is_tensor(img1) or img1.shape != img0.shape or img1.dtype != img0.dtype or img1.device != img0.device:
        raise ValueError(f'img1: expected the shape, dtype and device of img0 ({tuple(img0.shape)} {img0.dtype} {img0.device})')
    dev = img0.device
    _check_flow(flow_fwd, b, h, w, 'flow_fwd', dev)
    _check_flow(flow_bwd, b, h, w, 'flow_bwd', dev)
    _check_splat_size(h, w)
    t = _times32(times)
    t1 = np.float32(1.0) - t
    _hole_threshold(min_weight)
    occ_fwd, occ_bwd = _check_plane(occ_fwd, b, h, w, 'occ_fwd', dev), _check_plane(occ_bwd, b, h, w, 'occ_bwd', dev)
    if not img0.is_cuda:
        frames, holes = synthesize_host(img0, img1, splat_accumulate_host(flow_fwd, t), splat_accumulate_host(flow_bwd, t1), t,
                                        occ_fwd, occ_bwd, min_weight)
        return (frames, holes) if return_holes else frames
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    img0, img1 = img0.contiguous(), img1.contiguous()
    acc, _, _ = splat_accumulators(flow_fwd.float().contiguous(), t, flow_bwd.float().contiguous(), t1, min_weight=min_weight)
    k = t.size
    tarr, tptr = _host_times([t, t1])
    with torch.cuda.device(dev):
        out = torch.empty((b, k, h, w, 3), dtype=torch.uint8, device=dev)
        holes = torch.empty((b, k, h, w), dtype=torch.uint8, device=dev) if return_holes else None
        _abi.check(lib.um_frame_synthesize(img0.data_ptr(), img1.data_ptr(), layout, _ptr(occ_fwd), _ptr(occ_bwd), tptr, acc.data_ptr(),
                                           acc.numel() * 8, out.data_ptr(), _ptr(holes), b, k, h, w, float(min_weight), _stream()),
                   'um_frame_synthesize')
    return (out, holes.bool()) if return_holes else out


def between_times(k):
    """The times ``j / (k + 1)``, j = 1 .. k, of ``k`` evenly spaced in-between frames."""
    return [j / (k + 1) for j in range(1, int(k) + 1)]
