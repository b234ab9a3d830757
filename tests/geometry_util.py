"""Shared inputs of the geometry tests and of ``tests/golden/make_golden_geometry.py``: analytic plane scenes seen from posed pinhole
cameras, disparity pairs, and the fp64 evaluations the kernels and the fp32 host restatement are compared with."""
import math

import torch

from unimatch_amd import geometry

SHAPES = ((3, 33, 47), (2, 64, 97), (1, 5, 3), (1, 16, 64))      # odd sizes | W no multiple of 64 | less than a wave | one wave per row


def intrinsics_for(h, w):
    return torch.tensor([[0.9 * w, 0., (w - 1) / 2.], [0., 0.9 * w, (h - 1) / 2.], [0., 0., 1.]], dtype=torch.float64)


def rotation(axis, angle):
    """Rodrigues rotation matrix, float64."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    kx = torch.tensor([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * kx + (1 - math.cos(angle)) * (kx @ kx)


def rigid(axis, angle, t):
    p = torch.eye(4, dtype=torch.float64)
    p[:3, :3] = rotation(axis, angle)
    p[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return p


def plane_depth(normal, offset, k, h, w):
    """Depth map (float64) of the plane ``normal . X = offset`` (camera coordinates) seen through intrinsics ``k``."""
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    rays = torch.linalg.inv(k) @ torch.stack([gx, gy, torch.ones_like(gx)], 0).flatten(1)
    return (offset / (normal @ rays)).view(h, w)


def plane_in(pose, normal, offset):
    """The plane ``normal . X = offset`` in the coordinates ``X' = R X + t`` of ``pose``."""
    n = pose[:3, :3] @ normal
    return n, offset + n @ pose[:3, 3]


def plane_pair(seed, b, h, w, noise=0.008, block=True, invalid=True):
    """``b`` reference / source view pairs of one plane each: float32 ``(depth_ref, depth_src, intrinsics [b,3,3], pose [b,4,4])``
    with the ref -> src pose.  Each map is multiplied by ``1 + noise * randn``; ``block``: a quarter (of the height and of the width)
    of the source map is scaled by 1.5; ``invalid``: a few pixels are 0, NaN and inf."""
    g = torch.Generator().manual_seed(seed)
    k = intrinsics_for(h, w)
    refs, srcs, poses = [], [], []
    for i in range(b):
        pose = rigid((0.2, 1.0, 0.1 * i), 0.03, (0.15, -0.04 + 0.02 * i, 0.02))
        normal = torch.tensor([0.1, -0.2 + 0.1 * i, 1.0], dtype=torch.float64)
        normal = normal / normal.norm()
        ref = plane_depth(normal, 2.0, k, h, w)
        src = plane_depth(*plane_in(pose, normal, 2.0), k, h, w)
        ref = ref * (1 + noise * torch.randn(h, w, generator=g, dtype=torch.float64))
        src = src * (1 + noise * torch.randn(h, w, generator=g, dtype=torch.float64))
        if block:
            y0, x0 = h // 3, w // 3
            src[y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 4)] *= 1.5
        if invalid and h * w >= 64:
            ref[1, 2], ref[h // 2, w // 2], ref[h - 2, 3], ref[2, w - 3] = 0., float('nan'), float('inf'), -1.
            src[h // 2 + 1, w // 2 - 4], src[3, w // 2], src[h - 3, w // 2 + 2] = float('nan'), 0., float('inf')
        refs.append(ref)
        srcs.append(src)
        poses.append(pose)
    return (torch.stack(refs, 0).float(), torch.stack(srcs, 0).float(), k.float()[None].repeat(b, 1, 1).contiguous(),
            torch.stack(poses, 0).float())


def cam_fp64(intrinsics, pose):
    """``(cam_fwd, cam_inv)`` float64 ``[B, 30]`` of the float32 inputs, with LU inverses in float64 (no closed form, no rounding)."""
    k, p = intrinsics.double(), pose.double()
    out = []
    for q in (p, torch.linalg.inv(p)):
        out.append(torch.cat([torch.linalg.inv(k).flatten(1), q[:, :3, :3].flatten(1), q[:, :3, 3], k.flatten(1)], 1))
    return out


def depth_check_fp64(depth_ref, depth_src, intrinsics, pose, px_thr=1.0, rel_thr=0.01):
    cam_fwd, cam_inv = cam_fp64(intrinsics, pose)
    return geometry.depth_consistency_host(depth_ref.double(), depth_src.double(), cam_fwd, cam_inv, px_thr, rel_thr)


def depth_check_fp32(depth_ref, depth_src, intrinsics, pose, px_thr=1.0, rel_thr=0.01):
    cam = geometry.cam_pack_host(intrinsics, pose, bidir=True)
    b = depth_ref.shape[0]
    return geometry.depth_consistency_host(depth_ref.float(), depth_src.float(), cam[:b], cam[b:], px_thr, rel_thr)


def margins(fp32, fp64):
    """Per quantity: 4 x the largest ``|fp32 host - fp64|`` over the pixels where both are finite."""
    out = []
    for a, b in zip(fp32[1:], fp64[1:]):
        both = torch.isfinite(a) & torch.isfinite(b)
        out.append(4.0 * (a.double() - b)[both].abs().max().item() if both.any() else 0.0)
    return out


def check_depth_result(got, fp64, margin, px_thr=1.0, rel_thr=0.01, cap=0.005):
    """The issue's assertions for one evaluation ``got = (occ, err_px, err_rel)`` against ``fp64``: errors within the margins where
    finite and +inf exactly where fp64 says so; masks differ only within a margin of a threshold, on at most ``cap`` of the pixels.
    Returns the number of differing mask pixels."""
    occ, epx, erel = (t.detach().cpu().double() for t in got)
    occ64, epx64, erel64 = fp64
    for name, a, b, m in (('err_px', epx, epx64, margin[0]), ('err_rel', erel, erel64, margin[1])):
        assert torch.equal(torch.isinf(a) & (a > 0), torch.isinf(b) & (b > 0)), name
        assert not torch.isnan(a).any(), name
        fin = torch.isfinite(b)
        worst = (a - b)[fin].abs().max().item() if fin.any() else 0.0
        assert worst <= m, (name, worst, m)
    off = occ != occ64
    near = ((epx64 - px_thr).abs() <= margin[0]) | ((erel64 - rel_thr).abs() <= margin[1])
    assert not (off & ~near).any(), int((off & ~near).sum())
    assert int(off.sum()) <= cap * occ.numel(), (int(off.sum()), occ.numel())
    return int(off.sum())


def disparity_pair(seed, b, h, w, band=True):
    """Smooth positive left / right disparities that mostly agree, with inconsistent patches and (``band``) a band of columns whose
    match lies far out of frame."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b, 1, max(2, h // 8), max(2, w // 8), generator=g)
    dl = (torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True)[:, 0] * 0.15 * w + 0.5).float()
    dr = dl + 0.05 * torch.randn(b, h, w, generator=g)
    bad = torch.rand(b, h, w, generator=g) < 0.15
    dr = torch.where(bad, dr + 3.0 * torch.randn(b, h, w, generator=g), dr).float()
    if band:
        dl[:, :, : max(1, w // 8)] += 3.0 * w
        dr[:, :, -max(1, w // 10):] += 2.5 * w
    return dl.contiguous(), dr.contiguous()


def disparity_flows(dl, dr):
    """The flows the left / right check is defined on: ``fwd = (-dL, 0)``, ``bwd = (+dR, 0)``."""
    zero = torch.zeros_like(dl)
    return torch.stack([-dl, zero], 1), torch.stack([dr, zero], 1)


def occ_margins(fwd, bwd, alpha=0.01, beta=0.5):
    """fp64 restatement of the flow check: (|fwd + bwd(p + fwd)| - thr, |bwd + fwd(p + bwd)| - thr, thr) per pixel."""
    from unimatch_amd.model import _warp
    f, b = fwd.double().cpu(), bwd.double().cpu()
    thr = alpha * (torch.norm(f, dim=1) + torch.norm(b, dim=1)) + beta
    return torch.norm(f + _warp(b, f), dim=1) - thr, torch.norm(b + _warp(f, b), dim=1) - thr, thr


def check_occ(got, want, margin, thr):
    """Every pixel where ``got`` and ``want`` disagree lies within 1e-4 thr of the threshold (fp64)."""
    off = got.cpu().double() != want.double()
    assert (margin[off].abs() <= 1e-4 * thr[off]).all(), (int(off.sum()), margin[off].abs().max().item())
    return int(off.sum())
