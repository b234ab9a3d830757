"""Cross-view consistency masks and fused point clouds: what a caller does with the disparities / depths of several views.

  disparity_consistency_check(disp_left, disp_right, alpha, beta)      left / right occlusion masks of a rectified pair: the reference's
                                                                       forward_backward_consistency_check (unimatch/geometry.py:75-96)
                                                                       on the flows (-disp_left, 0) and (+disp_right, 0)
  depth_consistency_check(depth_ref, depth_src, intrinsics, pose, ..)  round trip of every reference pixel through the source view
                                                                       (back_project, camera_transform, reproject: geometry.py:99-154)
  back_project_points(depth, intrinsics, poses, keep, colors, ..)      world-space points (+ colours) of the selected pixels, in
                                                                       ascending (b, y, x) order
  fuse_depth_sequence(depths, intrinsics, poses, colors, ..)           every frame of a posed video checked against its neighbours,
                                                                       the consistent pixels fused into one cloud

``fuse_depth_sequence`` concatenates: every kept pixel of every frame is a point of its own.  Volumetric fusion of the same depths --
one voxel grid that averages them across frames, with ``keep`` or a confidence as the weight -- is :mod:`unimatch_amd.fusion`
(``TSDFVolume``, ``fuse_depth_sequence_tsdf``; ``csrc/fusion.hip``), which takes its bounds from ``back_project_points``.

CUDA tensors run on the HIP kernels of ``csrc/geometry.hip`` (``um_disp_consistency``, ``um_depth_consistency``, ``um_points_pack``),
with the camera records of ``um_depth_cam_pack`` and the relative poses of ``um_relative_pose_pairs``: no ``torch.inverse``, no
``grid_sample``, no boolean indexing, and one host synchronisation per cloud (the read of the point count).  Host tensors run the
restatement below, written operation by operation in the order and the precision (float32) of the kernels; the CPU tests pin it against
fixtures minted from the reference.  There is no silent fallback from one to the other.  (The ``*_host`` functions are plain torch
compositions and follow their inputs' device and dtype: the tests evaluate them in float64, ``tools/bench_geometry.py`` times them on
the GPU as the baseline of the kernels.)

Camera record (``[B, 30]``): ``Kinv | R | t | K``, row major -- K^-1 and, for the inverse pose, A^-1 by the adjugate in float64 rounded
once, ``t' = -A^-1 t`` in float32.
"""
import torch

_hip_ops = None


def _hip():
    global _hip_ops
    if _hip_ops is None:
        from .ops import HipOps            # raises when the HIP extension or the GPU is missing: there is no silent fallback
        _hip_ops = HipOps()
    return _hip_ops


# ------------------------------------------------------------------ host restatement: camera records
def _inv3_host(m):
    """``[B, 3, 3]`` -> its inverse in float64 by the adjugate (``inv3`` of csrc/upsample.hip); all NaN where singular."""
    m = m.double()
    a, b, c, d, e, f, g, h, i = (m[:, r, s] for r in range(3) for s in range(3))
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * c00 + b * c01 + c * c02
    inv_det = torch.where(det != 0, 1.0 / det, torch.full_like(det, float('nan')))
    rows = [c00, c * h - b * i, b * f - c * e, c01, a * i - c * g, c * d - a * f, c02, b * g - a * h, a * e - b * d]
    return torch.stack([r * inv_det for r in rows], 1).view(-1, 3, 3)


def cam_pack_host(intrinsics, pose, bidir=False):
    """``um_depth_cam_pack`` at ``stride_div = 1`` on the host: ``[B or 2B, 30]`` float32 from intrinsics ``[B, 3, 3]`` and pose
    ``[B, 4, 4]``; with ``bidir`` the second half carries the inverse pose."""
    k, p = intrinsics.float(), pose.float()
    kinv = _inv3_host(k).float()
    r, t = p[:, :3, :3], p[:, :3, 3]
    recs = [torch.cat([kinv.flatten(1), r.flatten(1), t, k.flatten(1)], 1)]
    if bidir:
        ri = _inv3_host(r).float()
        ti = -((ri[:, :, 0] * t[:, None, 0] + ri[:, :, 1] * t[:, None, 1]) + ri[:, :, 2] * t[:, None, 2])
        recs.append(torch.cat([kinv.flatten(1), ri.flatten(1), ti, k.flatten(1)], 1))
    return torch.cat(recs, 0).contiguous()


def relative_pose_pairs_host(poses):
    """``um_relative_pose_pairs`` on the host: ``rel[t] = inv(poses[t + 1]) @ poses[t]``, formed in float64 from the float32 poses
    (affine: the bottom row is not read) and rounded once; the bottom row is exactly 0 0 0 1."""
    p = poses.float().double()
    ai = _inv3_host(p[1:, :3, :3])
    rel = torch.zeros(p.shape[0] - 1, 4, 4, dtype=torch.float64)
    rel[:, :3, :3] = ai @ p[:-1, :3, :3]
    rel[:, :3, 3] = (ai @ (p[:-1, :3, 3] - p[1:, :3, 3])[..., None])[..., 0]
    rel[:, 3, 3] = 1.0
    return rel.float()


def _lift(cam, u, v, depth):
    """``X = R (depth Kinv (u, v, 1)) + t`` per pixel, in ``cam``'s dtype and the kernels' operation order (``cam_lift``)."""
    c = [cam[:, j].view(-1, 1, 1) for j in range(30)]
    r0, r1, r2 = (c[0] * u + c[1] * v + c[2]) * depth, (c[3] * u + c[4] * v + c[5]) * depth, (c[6] * u + c[7] * v + c[8]) * depth
    return (c[9] * r0 + c[10] * r1 + c[11] * r2 + c[18], c[12] * r0 + c[13] * r1 + c[14] * r2 + c[19],
            c[15] * r0 + c[16] * r1 + c[17] * r2 + c[20])


def _project(cam, x, y, z):
    """``(K X)_xy / max((K X)_z, 1e-3)`` (``cam_project``; geometry.py:132-154)."""
    c = [cam[:, j].view(-1, 1, 1) for j in range(30)]
    zz = (c[27] * x + c[28] * y + c[29] * z).clamp(min=1e-3)
    return (c[21] * x + c[22] * y + c[23] * z) / zz, (c[24] * x + c[25] * y + c[26] * z) / zz


def _pixel_grid(h, w, dtype, device=None):
    gy, gx = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device), indexing='ij')
    return gx[None], gy[None]


def reproject_host(depth_ref, cam_fwd):
    """Steps 1-2 of the depth check: ``(u, v, in_view)`` of every reference pixel in the source view."""
    b, h, w = depth_ref.shape
    gx, gy = _pixel_grid(h, w, depth_ref.dtype, depth_ref.device)
    u, v = _project(cam_fwd, *_lift(cam_fwd, gx, gy, depth_ref))
    return u, v, (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)


# ------------------------------------------------------------------ host restatement: the three operations
def disparity_consistency_host(disp_left, disp_right, alpha=0.01, beta=0.5):
    """``um_disp_consistency`` step by step, in the dtype of the inputs."""
    dl, dr = disp_left, disp_right
    b, h, w = dl.shape
    x = torch.arange(w, dtype=dl.dtype, device=dl.device).view(1, 1, w)

    def row_sample(rows, dx):
        px = x + dx
        gx = 2.0 * px / (w - 1) - 1.0
        ix = ((gx + 1.0) / 2.0) * (w - 1)
        fx0 = torch.floor(ix)
        fx1 = fx0 + 1.0
        w0, w1 = fx1 - ix, ix - fx0
        x0 = torch.nan_to_num(fx0, nan=-2.0).clamp(-2.0, w + 1.0).long()
        out = torch.zeros_like(rows)
        for xi, wt in ((x0, w0), (x0 + 1, w1)):
            inside = (xi >= 0) & (xi < w)
            val = rows.gather(2, xi.clamp(0, w - 1))
            out = torch.where(inside, out + val * wt, out)
        return out

    fu, bu = -dl, dr
    thr = alpha * (torch.sqrt(fu * fu) + torch.sqrt(bu * bu)) + beta
    du, eu = fu + row_sample(dr, fu), bu - row_sample(dl, bu)
    return (torch.sqrt(du * du) > thr).to(dl.dtype), (torch.sqrt(eu * eu) > thr).to(dl.dtype)


def depth_consistency_host(depth_ref, depth_src, cam_fwd, cam_inv, px_thr=1.0, rel_thr=0.01):
    """``um_depth_consistency`` step by step, in the dtype of the inputs: ``(occ, err_px, err_rel)``."""
    d, src = depth_ref, depth_src
    b, h, w = d.shape
    gx, gy = _pixel_grid(h, w, d.dtype, d.device)
    u, v, in_view = reproject_host(d, cam_fwd)
    inside = torch.isfinite(d) & (d > 0) & in_view
    zero = torch.zeros_like(d)
    fx0, fy0 = torch.where(inside, torch.floor(u), zero), torch.where(inside, torch.floor(v), zero)
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    ax, ay = torch.where(inside, u - fx0, zero), torch.where(inside, v - fy0, zero)
    flat = src.flatten(1)
    ok, s = inside, zero
    for yy, xx, wt in ((y0, x0, (1.0 - ax) * (1.0 - ay)), (y0, x1, ax * (1.0 - ay)), (y1, x0, (1.0 - ax) * ay), (y1, x1, ax * ay)):
        tap = flat.gather(1, (yy * w + xx).flatten(1)).view(b, h, w)
        used = wt != 0
        ok = ok & (~used | (torch.isfinite(tap) & (tap > 0)))
        s = torch.where(used, s + wt * tap, s)
    safe_u, safe_v, safe_s = torch.where(ok, u, zero), torch.where(ok, v, zero), torch.where(ok, s, zero)
    x, y, z = _lift(cam_inv, safe_u, safe_v, safe_s)
    bu, bv = _project(cam_inv, x, y, z)
    ex, ey = bu - gx, bv - gy
    inf = torch.full_like(d, float('inf'))
    err_px = torch.where(ok, torch.sqrt(ex * ex + ey * ey), inf)
    err_rel = torch.where(ok, (z - d).abs() / d, inf)
    occ = (~((err_px < px_thr) & (err_rel < rel_thr))).to(d.dtype)
    return occ, err_px, err_rel


def points_selection_host(depth, keep=None, min_depth=0., max_depth=float('inf'), stride=1):
    """The boolean ``[B, H, W]`` selection of ``um_points_pack``."""
    b, h, w = depth.shape
    sel = torch.isfinite(depth) & (depth > min_depth) & (depth < max_depth)
    grid = torch.zeros(h, w, dtype=torch.bool, device=depth.device)
    grid[::stride, ::stride] = True
    sel = sel & grid[None]
    return sel if keep is None else sel & (keep != 0)


def points_pack_host(depth, cam_world, keep=None, colors=None, min_depth=0., max_depth=float('inf'), stride=1):
    """``um_points_pack`` step by step, in the dtype of ``depth``: ``(xyz [N, 3], rgb [N, 3] or None)`` in ``(b, y, x)`` order."""
    b, h, w = depth.shape
    sel = points_selection_host(depth, keep, min_depth, max_depth, stride)
    gx, gy = _pixel_grid(h, w, depth.dtype, depth.device)
    xyz = torch.stack(_lift(cam_world, gx, gy, torch.where(sel, depth, torch.zeros_like(depth))), -1)[sel]
    return xyz, None if colors is None else colors[sel]


# ------------------------------------------------------------------ public functions
def _expand_intrinsics(intrinsics, n, what):
    if intrinsics.dim() != 3 or tuple(intrinsics.shape[1:]) != (3, 3) or intrinsics.shape[0] not in (1, n):
        raise ValueError(f'{what}: expected intrinsics [1 or {n}, 3, 3], got {tuple(intrinsics.shape)}')
    return intrinsics.float().expand(n, 3, 3).contiguous()


def _check_poses(pose, n, what):
    if pose.dim() != 3 or tuple(pose.shape) != (n, 4, 4):
        raise ValueError(f'{what}: expected poses [{n}, 4, 4], got {tuple(pose.shape)}')
    return pose.float().contiguous()


def _same_device(what, first, **others):
    for name, t in others.items():
        if t is not None and t.device != first.device:
            raise ValueError(f'{what}: {name} is on {t.device}, the depth on {first.device}: there is no silent transfer')


def _cam_pack(intrinsics, pose, bidir):
    return _hip().depth_cam(intrinsics, pose, 1.0, bidir=bidir) if intrinsics.is_cuda else cam_pack_host(intrinsics, pose, bidir)


def disparity_consistency_check(disp_left, disp_right, alpha=0.01, beta=0.5):
    """``(occ_left, occ_right)`` ``[B, H, W]`` float in {0, 1} (1 = occluded) of the disparities ``disp_left``, ``disp_right``
    ``[B, H, W]`` of a rectified pair: the left pixel ``x`` matches the right pixel ``x - dL(x)``, and it is occluded where the right
    view's disparity sampled there disagrees, ``|dL - dR(x - dL)| > alpha (|dL| + |dR|) + beta`` (both magnitudes at ``x`` itself, as in
    the flow check); the right view likewise at ``x + dR(x)``.  The defaults are the flow check's, parameters rather than claims."""
    if disp_left.dim() != 3 or disp_right.shape != disp_left.shape or disp_left.shape[-1] < 2:
        raise ValueError(f'expected two [B, H, W >= 2] disparities of one shape, got {tuple(disp_left.shape)} and {tuple(disp_right.shape)}')
    _same_device('disparity_consistency_check', disp_left, disp_right=disp_right)
    if disp_left.is_cuda:
        with torch.cuda.device(disp_left.device):
            return _hip().disp_consistency(disp_left.float(), disp_right.float(), alpha, beta)
    return disparity_consistency_host(disp_left.float(), disp_right.float(), alpha, beta)


def depth_consistency_check(depth_ref, depth_src, intrinsics, pose, px_thr=1.0, rel_thr=0.01, return_errors=False):
    """``occ [B, H, W]`` float in {0, 1} (1 = inconsistent) of the metric depths ``depth_ref``, ``depth_src`` ``[B, H, W]`` of two
    views with ``intrinsics [1 or B, 3, 3]`` (both views) and the ref -> src ``pose [B, 4, 4]``: every reference pixel is lifted,
    moved into the source view and projected; the source depth sampled there (bilinear) is lifted and brought back with the inverse
    pose; the pixel is consistent iff it returns within ``px_thr`` pixels of where it started AND at a depth within ``rel_thr`` of its
    own.  Pixels with a non-finite or non-positive depth, out of the source view, or sampling such a source depth are inconsistent.
    ``return_errors``: ``(occ, err_px, err_rel)``, the errors ``+inf`` at those pixels."""
    if depth_ref.dim() != 3 or depth_src.shape != depth_ref.shape:
        raise ValueError(f'expected two [B, H, W] depths of one shape, got {tuple(depth_ref.shape)} and {tuple(depth_src.shape)}')
    b = depth_ref.shape[0]
    _same_device('depth_consistency_check', depth_ref, depth_src=depth_src, intrinsics=intrinsics, pose=pose)
    k, p = _expand_intrinsics(intrinsics, b, 'depth_consistency_check'), _check_poses(pose, b, 'depth_consistency_check')
    if depth_ref.is_cuda:
        with torch.cuda.device(depth_ref.device):
            cam = _cam_pack(k, p, True)
            return _hip().depth_consistency(depth_ref.float(), depth_src.float(), cam[:b], cam[b:], px_thr, rel_thr, return_errors)
    cam = _cam_pack(k, p, True)
    out = depth_consistency_host(depth_ref.float(), depth_src.float(), cam[:b], cam[b:], px_thr, rel_thr)
    return out if return_errors else out[0]


def back_project_points(depth, intrinsics, poses, keep=None, colors=None, min_depth=0., max_depth=float('inf'), stride=1):
    """``(xyz [N, 3] float32, rgb [N, 3] uint8 or None)``: the world points ``R (d Kinv p) + t`` of the selected pixels of
    ``depth [B, H, W]`` with ``intrinsics [1 or B, 3, 3]`` and camera-to-world ``poses [B, 4, 4]``, in ascending ``(b, y, x)`` order.
    A pixel is selected iff ``x % stride == 0 and y % stride == 0``, ``keep`` (``[B, H, W]``, non-zero = keep; ``None``: all) keeps it
    and its depth is finite with ``min_depth < d < max_depth``.  ``colors``: ``[B, H, W, 3]`` uint8.

    On the device this call makes ONE host synchronisation: the read of N, after which the results are sliced to N rows."""
    if depth.dim() != 3:
        raise ValueError(f'expected a [B, H, W] depth, got {tuple(depth.shape)}')
    b, h, w = depth.shape
    what = 'back_project_points'
    _same_device(what, depth, intrinsics=intrinsics, poses=poses, keep=keep, colors=colors)
    k, p = _expand_intrinsics(intrinsics, b, what), _check_poses(poses, b, what)
    if int(stride) < 1:
        raise ValueError(f'{what}: stride must be >= 1, got {stride}')
    if keep is not None and keep.shape != depth.shape:
        raise ValueError(f'{what}: expected keep {tuple(depth.shape)}, got {tuple(keep.shape)}')
    if colors is not None and (tuple(colors.shape) != (b, h, w, 3) or colors.dtype != torch.uint8):
        raise ValueError(f'{what}: expected colors uint8 {(b, h, w, 3)}, got {colors.dtype} {tuple(colors.shape)}')
    keep = None if keep is None else keep.float()
    if depth.is_cuda:
        with torch.cuda.device(depth.device):
            xyz, rgb, count = _hip().points_pack(depth.float(), _cam_pack(k, p, False), keep, colors, min_depth, max_depth, int(stride))
            n = int(count.item())                                      # the one synchronisation
            return xyz[:n], None if rgb is None else rgb[:n]
    return points_pack_host(depth.float(), _cam_pack(k, p, False), keep, colors, min_depth, max_depth, int(stride))


def fuse_depth_sequence(depths, intrinsics, poses, colors=None, px_thr=1.0, rel_thr=0.01, min_views=1, confidence=None,
                        min_confidence=0., **points_kw):
    """The consistency-filtered world point cloud of a posed video: ``dict(xyz [N, 3], rgb [N, 3] or None, keep [T, H, W])``.

    ``depths [T, H, W]`` metric, ``intrinsics [1 or T, 3, 3]`` (row ``t`` serves both views of the pair ``(t, t + 1)``),
    ``poses [T, 4, 4]`` camera-to-world, ``T >= 2``.  Every frame is checked (:func:`depth_consistency_check`) against each adjacent
    frame, ``t - 1`` and ``t + 1``; ``keep[t]`` is 1 where at least ``min_views`` of its neighbours are consistent (the first and the
    last frame have one neighbour: ``min_views=2`` drops them).  All ``2 (T - 1)`` directed checks are one launch; the relative poses
    come from ``um_relative_pose_pairs`` and one bidirectional camera pack supplies the forward records and, rotated by ``T - 1``, the
    inverse ones.  ``confidence [T, H, W]`` (at the depths' size, e.g. the plane sweep's ``peak_mass`` brought to image size by
    ``confidence.confidence_to_image_size``): ``keep`` is additionally 0 where ``confidence < min_confidence`` -- the one filter that
    also serves a frame without a consistent neighbour; without it the result is unchanged.  ``points_kw``: ``min_depth``, ``max_depth``, ``stride`` of :func:`back_project_points`, whose one synchronisation is
    the only one here."""
    if depths.dim() != 3 or depths.shape[0] < 2:
        raise ValueError(f'expected depths [T >= 2, H, W], got {tuple(depths.shape)}')
    t = depths.shape[0]
    what = 'fuse_depth_sequence'
    _same_device(what, depths, intrinsics=intrinsics, poses=poses, colors=colors, confidence=confidence)
    if confidence is not None and tuple(confidence.shape) != tuple(depths.shape):
        raise ValueError(f'{what}: confidence {tuple(confidence.shape)} is not at the depths\' size {tuple(depths.shape)}')
    k, p = _expand_intrinsics(intrinsics, t, what), _check_poses(poses, t, what)
    depths = depths.float()
    ref, src = torch.cat([depths[:-1], depths[1:]], 0), torch.cat([depths[1:], depths[:-1]], 0)
    if depths.is_cuda:
        with torch.cuda.device(depths.device):
            cam = _cam_pack(k[:-1], _hip().relative_pose_pairs(p), True)
            occ = _hip().depth_consistency(ref, src, cam, cam.roll(t - 1, 0), px_thr, rel_thr)
    else:
        cam = _cam_pack(k[:-1], relative_pose_pairs_host(p), True)
        occ = depth_consistency_host(ref, src, cam, cam.roll(t - 1, 0), px_thr, rel_thr)[0]
    votes = torch.zeros_like(depths)
    votes[:-1] += 1.0 - occ[:t - 1]                                    # frame t against t + 1
    votes[1:] += 1.0 - occ[t - 1:]                                     # frame t + 1 against t
    keep = (votes >= float(min_views)).float()
    if confidence is not None:
        keep = keep * (confidence >= float(min_confidence)).float()
    xyz, rgb = back_project_points(depths, k, p, keep=keep, colors=colors, **points_kw)
    return {'xyz': xyz, 'rgb': rgb, 'keep': keep}
