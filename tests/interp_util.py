"""Shared by the frame-synthesis tests: an INDEPENDENT oracle of ``interp.splat_flow`` / ``interp.interpolate_frames`` -- a plain
per-pixel Python loop in float64, written from the specification and sharing no code with the restatement in ``unimatch_amd/interp.py``
-- and the seeded inputs of both test files.

The oracle's only float32 steps are the ones the specification names as such: the landing point ``(float)x + t u``, the four tap
products, their product with the weight, the two quantisations, and the rounding of the averaged flow to float32.  The float32 times
(t and 1 - t) are the inputs' own.  Everything of the synthesis (positions, samples, weights, blend) is float64, so a frame value
that lies within ``EDGE`` of a rounding boundary ``n + 0.5`` is excluded from the exact comparison (and counted)."""
import math

import numpy as np
import torch

EDGE = 1e-3               # distance of a float64 blend from n + 0.5 below which float32 may round the other way
EDGE_SHARE = 0.02         # at most this share of a case's values may be that close (a condition on the seeded inputs)
f32 = np.float32


# ------------------------------------------------------------------ seeded inputs
def smooth_pair(b, h, w, seed, amp=2.5):
    """``(fwd, bwd)`` ``[b, 2, h, w]`` float32: a smooth forward flow and a backward flow that roughly cancels it."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(b, 2, 3, 4, generator=g)
    fwd = torch.nn.functional.interpolate(coarse, (h, w), mode='bilinear', align_corners=True) * amp + torch.tensor([0.8, -0.45]).view(1, 2, 1, 1)
    bwd = -fwd + 0.3 * torch.nn.functional.interpolate(torch.randn(b, 2, 3, 4, generator=g), (h, w), mode='bilinear', align_corners=True)
    return fwd.float().contiguous(), bwd.float().contiguous()


def texture(b, h, w, seed):
    """A seeded uint8 image ``[b, h, w, 3]``."""
    return torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def as_float_layout(img_u8):
    return img_u8.permute(0, 3, 1, 2).float().contiguous()


def masks(b, h, w, seed):
    """Two seeded occlusion masks ``[b, h, w]`` in {0, 1}, about a fifth occluded, in blobs."""
    g = torch.Generator().manual_seed(seed)
    blobs = torch.nn.functional.interpolate(torch.rand(2 * b, 1, 3, 4, generator=g), (h, w), mode='bilinear', align_corners=True)[:, 0]
    m = (blobs > 0.62).float()
    return m[:b].contiguous(), m[b:].contiguous()


def bad_inputs(fwd, bwd, seed):
    """Copies of the flows with NaN, +-inf and 1e9 planted, and a weight plane with NaN / 0 / -1 / 7 / inf planted."""
    b, _, h, w = fwd.shape
    g = torch.Generator().manual_seed(seed)
    fwd, bwd = fwd.clone(), bwd.clone()
    weight = 0.25 + 0.75 * torch.rand(b, h, w, generator=g)
    vals = (float('nan'), float('inf'), float('-inf'), 1e9, -1e9, 40000.0)
    for i, v in enumerate(vals):
        fwd.view(b, 2, -1)[0, i % 2, (3 * i + 1) % (h * w)] = v
        bwd.view(b, 2, -1)[b - 1, (i + 1) % 2, (5 * i + 2) % (h * w)] = v
    for i, v in enumerate((float('nan'), 0.0, -1.0, 7.0, float('inf'), float('-inf'))):
        weight.view(b, -1)[i % b, (7 * i + 3) % (h * w)] = v
    return fwd, bwd, weight.contiguous()


# ------------------------------------------------------------------ the oracle
def _rint(v):
    """Round half to even, as C's rint in the default mode (Python's round does the same on floats)."""
    return int(round(float(v)))


def oracle_accumulate(flow, times, weight=None):
    """``S [B, K, 3, H, W]`` as Python ints in an int64 array: the integer sums of the specification, pixel by pixel."""
    flow = flow.numpy().astype(np.float32)
    b, _, h, w = flow.shape
    wgt = None if weight is None else weight.numpy().astype(np.float32)
    acc = np.zeros((b, len(times), 3, h, w), dtype=np.int64)
    for bi in range(b):
        for y in range(h):
            for x in range(w):
                u, v = flow[bi, 0, y, x], flow[bi, 1, y, x]
                if not (math.isfinite(u) and math.isfinite(v)) or abs(u) > 32768 or abs(v) > 32768:
                    continue
                g = f32(1)
                if wgt is not None:
                    g = wgt[bi, y, x]
                    if not math.isfinite(g) or g <= 0:
                        continue
                    g = min(g, f32(1))
                uq, vq = _rint(f32(u * f32(256))), _rint(f32(v * f32(256)))
                for k, t in enumerate(times):
                    t = f32(t)
                    X, Y = f32(f32(x) + f32(t * u)), f32(f32(y) + f32(t * v))
                    x0, y0 = math.floor(X), math.floor(Y)
                    ax, ay = f32(X - f32(x0)), f32(Y - f32(y0))
                    one = f32(1)
                    taps = ((y0, x0, f32(f32(one - ax) * f32(one - ay))), (y0, x0 + 1, f32(ax * f32(one - ay))),
                            (y0 + 1, x0, f32(f32(one - ax) * ay)), (y0 + 1, x0 + 1, f32(ax * ay)))
                    for yy, xx, wt in taps:
                        if 0 <= yy < h and 0 <= xx < w:
                            wq = _rint(f32(f32(wt * g) * f32(65536)))
                            acc[bi, k, 0, yy, xx] += wq
                            acc[bi, k, 1, yy, xx] += wq * uq
                            acc[bi, k, 2, yy, xx] += wq * vq
    return acc


def oracle_average(acc, min_weight=1.0 / 256):
    """``(flow [B, K, 2, H, W] float64 holding float32 values, hole [B, K, H, W] bool)``."""
    thr = max(1, _rint(f32(f32(min_weight) * f32(65536))))
    sw = acc[:, :, 0]
    hole = sw < thr
    den = np.where(hole, 1, sw).astype(np.float64)
    flow = np.stack([acc[:, :, 1] / den / 256.0, acc[:, :, 2] / den / 256.0], 2).astype(np.float32).astype(np.float64)
    flow[np.broadcast_to(hole[:, :, None], flow.shape)] = 0.0
    return flow, hole


def _bilinear64(img, x, y, border):
    """float64 bilinear sample of ``img [h, w, c]`` at (x, y): border clamping, or zeros outside."""
    h, w = img.shape[:2]
    if border:
        x, y = min(max(x, 0.0), w - 1.0), min(max(y, 0.0), h - 1.0)
    x0, y0 = math.floor(x), math.floor(y)
    out = np.zeros(img.shape[2], dtype=np.float64)
    for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
        wt = (1.0 - abs(x - xx)) * (1.0 - abs(y - yy))
        if 0 <= yy < h and 0 <= xx < w and wt > 0:
            out += wt * img[yy, xx]
    return out


def oracle_frames(img0, img1, fwd, bwd, times, occ_fwd=None, occ_bwd=None, min_weight=1.0 / 256):
    """``(blend [B, K, H, W, 3] float64 BEFORE rounding, holes [B, K, H, W] bool)``; ``img0``, ``img1`` ``[B, H, W, 3]`` uint8."""
    t32 = [f32(t) for t in times]
    t1_32 = [f32(f32(1) - t) for t in t32]
    A, hole_a = oracle_average(oracle_accumulate(fwd, t32), min_weight)
    B, hole_b = oracle_average(oracle_accumulate(bwd, t1_32), min_weight)
    i0, i1 = img0.numpy().astype(np.float64), img1.numpy().astype(np.float64)
    o_f = None if occ_fwd is None else occ_fwd.numpy().astype(np.float64)[..., None]
    o_b = None if occ_bwd is None else occ_bwd.numpy().astype(np.float64)[..., None]
    b, h, w = i0.shape[:3]
    blend = np.zeros((b, len(times), h, w, 3))
    holes = np.zeros((b, len(times), h, w), dtype=bool)
    for bi in range(b):
        for k in range(len(times)):
            t, t1 = float(t32[k]), float(t1_32[k])
            for y in range(h):
                for x in range(w):
                    va, vb = not hole_a[bi, k, y, x], not hole_b[bi, k, y, x]
                    a, bb = A[bi, k, :, y, x], B[bi, k, :, y, x]
                    if va and vb:
                        m = 0.5 * (a - bb)
                    elif va:
                        m = a
                    elif vb:
                        m = -bb
                    else:
                        m = np.zeros(2)
                        holes[bi, k, y, x] = True
                    x0, y0, x1, y1 = x - t * m[0], y - t * m[1], x + t1 * m[0], y + t1 * m[1]
                    v0 = 1.0 if (0 <= x0 <= w - 1 and 0 <= y0 <= h - 1) else 0.0
                    v1 = 1.0 if (0 <= x1 <= w - 1 and 0 <= y1 <= h - 1) else 0.0
                    c0, c1 = _bilinear64(i0[bi], x0, y0, True), _bilinear64(i1[bi], x1, y1, True)
                    o0 = 0.0 if o_f is None else _bilinear64(o_f[bi], x0, y0, False)[0]
                    o1 = 0.0 if o_b is None else _bilinear64(o_b[bi], x1, y1, False)[0]
                    w0, w1 = t1 * v0 * (1.0 - o1), t * v1 * (1.0 - o0)
                    if w0 + w1 < 1e-6:
                        w0, w1 = t1, t
                    blend[bi, k, y, x] = (w0 * c0 + w1 * c1) / (w0 + w1)
    return blend, holes


def compare_rounded(got_u8, blend64):
    """``got`` (uint8) against ``rint(blend)`` wherever the float64 blend is farther than EDGE from a rounding boundary: returns the
    share of excluded values; asserts exact equality on the rest."""
    blend64 = np.asarray(blend64, dtype=np.float64)
    got = np.asarray(got_u8)
    near = np.abs(blend64 - np.floor(blend64) - 0.5) <= EDGE
    want = np.clip(np.rint(blend64), 0, 255).astype(np.uint8)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want) & ~near
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return float(near.mean())


def shift_bilinear64(img_u8, dx, dy):
    """float64 ``out(q) = bilinear(img, q - (dx, dy))`` of ``img [h, w, 3]`` with border clamping, and the mask of the pixels whose
    sample position is in frame."""
    img = np.asarray(img_u8).astype(np.float64)
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    inside = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = _bilinear64(img, x - dx, y - dy, True)
            inside[y, x] = 0 <= x - dx <= w - 1 and 0 <= y - dy <= h - 1
    return out, inside
