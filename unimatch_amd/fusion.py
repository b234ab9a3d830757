"""Volumetric (TSDF) fusion of posed depth maps: one voxel grid averages the per-frame depths, weighted, and yields one surface.

  TSDFVolume(origin, voxel_size, dims, trunc, max_weight, with_color)   the volume state and its three operations: ``integrate``,
                                                                        ``extract_points``, ``extract_mesh``, ``reset``
  volume_bounds(depths, intrinsics, poses, keep, ...)                   the axis-aligned box of the kept back-projected points
  fuse_depth_sequence_tsdf(depths, intrinsics, poses, colors, weight)   a posed video fused into one volume, in chunks of views, and
                                                                        its surface points: ``dict(xyz, rgb, volume)``

Where :func:`unimatch_amd.geometry.fuse_depth_sequence` concatenates every kept pixel of every frame (a surface seen by ten frames
appears ten times, with ten noise samples), the volume stays at a fixed size however long the video is, averages the depths across
frames and uses the confidence / consistency as a WEIGHT.

CUDA tensors run the kernels of ``csrc/fusion.hip`` (``um_tsdf_integrate``, ``um_tsdf_points``) with the camera records of
``um_depth_cam_pack``; host tensors run the ``*_host`` restatement below, written operation by operation in the kernels' order.  In
float32 the two are bitwise equal; the restatement follows the dtype of the volume it is given, so the tests evaluate it in float64 too
(``tools/bench_tsdf.py`` times it on the GPU as the baseline of the kernel).  There is no silent fallback from one to the other.

Volume state: ``tsdf [nz, ny, nx]`` in units of the truncation distance, in [-1, 1]; ``weight [nz, ny, nx]`` >= 0; ``color
[3, nz, ny, nx]`` running means in 0..255 (or ``None``); float32, x fastest, a fresh volume all zeros.  Voxel ``(i, j, k)`` has the world
centre ``(ox + (float)i voxel, oy + (float)j voxel, oz + (float)k voxel)``.

``integrate``, per voxel ``(x, y, z)`` and view (views in ascending order), with ``c`` the view's WORLD-TO-CAMERA record (the second half
of a bidirectional camera pack of the intrinsics and the camera-to-world pose):

 1. ``Xc_r = c[9+3r] x + c[10+3r] y + c[11+3r] z + c[18+r]``, summed left to right;
 2. ``zz = c[27] Xc_0 + c[28] Xc_1 + c[29] Xc_2``; skip the view unless ``zz > 1e-3``;
 3. ``u = (c[21] Xc_0 + c[22] Xc_1 + c[23] Xc_2) / zz``, ``v`` likewise with ``c[24..26]``;
 4. ``px = rint(u)``, ``py = rint(v)``: the nearest pixel (interpolating depth across a discontinuity would invent surfaces);
 5. skip unless ``0 <= px <= W - 1`` and ``0 <= py <= H - 1`` (a NaN position skips);
 6. ``d = depth[b, py, px]``; skip unless ``d`` is finite and ``min_depth < d < max_depth``;
 7. ``w = weight[b, py, px]`` (1 without weights); skip unless ``w`` is finite and ``w > 0``;
 8. ``sdf = d - Xc_2``; skip unless ``sdf >= -trunc``;
 9. ``f = min(1, sdf / trunc)``;
10. ``Wn = W + w``, ``tsdf = (tsdf W + f w) / Wn``;
11. each colour plane ``C = (C W + (float)colors w) / Wn``;
12. ``W = min(Wn, max_weight)``.

``extract_points``: candidates in ascending ``(k, j, i)``, then by axis x, y, z; the candidate of voxel ``p`` and axis ``a`` is the edge to
the neighbour ``n = p + e_a`` inside the volume, a crossing iff both weights are ``>= min_weight``, ``(tp < 0) != (tn < 0)`` and
``|tp| < 1``, ``|tn| < 1`` (which drops free-space-to-unseen jumps at occlusion borders).  With ``s = tp / (tp - tn)`` its point is
``X(p)`` with coordinate ``a`` increased by ``s voxel``, its colour ``rint(Cp + s (Cn - Cp))`` clamped to 0..255.

``extract_mesh`` (``csrc/tsdf_mesh.hip``, ``um_tsdf_mesh``): marching tetrahedra on the Kuhn split of every cell whose eight corners are
valid; the definition is written out at ``um_tsdf_mesh`` in ``include/unimatch_hip.h`` and restated by :func:`extract_mesh_host`.  Its
vertices on the axis edges are bit for bit points of ``extract_points``.
"""
import ctypes
import math

import numpy as np
import torch

from . import _abi, geometry


# ------------------------------------------------------------------ argument checks
def _f32(v):
    """A Python scalar as the C ABI receives it: rounded to float32 once."""
    return float(np.float32(v))


def _scalar(v, like):
    return torch.tensor(_f32(v), dtype=like.dtype, device=like.device)


def _check_dims(dims):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f'dims: expected (nx, ny, nz), all >= 1 with nx ny nz < 2^31, got {dims}')
    return dims


def _check_positive(**values):
    for name, v in values.items():
        if not _f32(v) > 0:
            raise ValueError(f'{name}: expected a value > 0, got {v!r}')


def _check_views(what, dev, depth, weight, colors):
    if not torch.is_tensor(depth) or depth.dim() != 3 or not depth.is_floating_point():
        raise ValueError(f'{what}: expected a floating-point [B, H, W] depth, got {tuple(getattr(depth, "shape", ()))}')
    b, h, w = depth.shape
    if weight is not None and (tuple(weight.shape) != (b, h, w) or not weight.is_floating_point()):
        raise ValueError(f'{what}: expected weight as floating-point {(b, h, w)}, got {tuple(weight.shape)} {weight.dtype}')
    if colors is not None and (tuple(colors.shape) != (b, h, w, 3) or colors.dtype != torch.uint8):
        raise ValueError(f'{what}: expected colors uint8 {(b, h, w, 3)}, got {colors.dtype} {tuple(colors.shape)}')
    for name, t in (('depth', depth), ('weight', weight), ('colors', colors)):
        if t is not None and t.device != dev:
            raise ValueError(f'{what}: {name} is on {t.device}, the volume on {dev}: there is no silent transfer')
    return b, h, w


# ------------------------------------------------------------------ host restatement
def voxel_projection_host(cam_view, origin, voxel, dims, dtype=torch.float32):
    """Steps 1-3 for every voxel and view, in ``dtype``: ``(Xc_2, zz, u, v)``, each ``[B, nz, ny, nx]``."""
    nx, ny, nz = dims
    cam = cam_view.to(dtype)
    vs = _scalar(voxel, cam)
    x = (_scalar(origin[0], cam) + torch.arange(nx, dtype=dtype, device=cam.device) * vs).view(1, 1, 1, nx)
    y = (_scalar(origin[1], cam) + torch.arange(ny, dtype=dtype, device=cam.device) * vs).view(1, 1, ny, 1)
    z = (_scalar(origin[2], cam) + torch.arange(nz, dtype=dtype, device=cam.device) * vs).view(1, nz, 1, 1)
    c = [cam[:, j].view(-1, 1, 1, 1) for j in range(30)]
    x0 = c[9] * x + c[10] * y + c[11] * z + c[18]
    x1 = c[12] * x + c[13] * y + c[14] * z + c[19]
    x2 = c[15] * x + c[16] * y + c[17] * z + c[20]
    zz = c[27] * x0 + c[28] * x1 + c[29] * x2
    return x2, zz, (c[21] * x0 + c[22] * x1 + c[23] * x2) / zz, (c[24] * x0 + c[25] * x1 + c[26] * x2) / zz


def integrate_host(tsdf, weight, color, depth, cam_view, weight_in=None, colors=None, *, origin, voxel, trunc, max_weight=64.,
                   min_depth=0., max_depth=float('inf')):
    """``um_tsdf_integrate`` step by step, in the dtype of ``tsdf``: the new ``(tsdf, weight, color)`` (the arguments are not written).
    The scalar parameters are rounded to float32 first, as the C ABI receives them."""
    nz, ny, nx = tsdf.shape
    b, h, w = depth.shape
    dt = tsdf.dtype
    depth = depth.to(dt)
    weight_in = None if weight_in is None else weight_in.to(dt)
    x2, zz, u, v = voxel_projection_host(cam_view, origin, voxel, (nx, ny, nz), dt)
    tr, mw, lo, hi = _scalar(trunc, tsdf), _scalar(max_weight, tsdf), _scalar(min_depth, tsdf), _scalar(max_depth, tsdf)
    one, eps = torch.ones((), dtype=dt, device=tsdf.device), _scalar(1e-3, tsdf)
    T, W = tsdf.clone(), weight.clone()
    C = None if color is None else [color[ch].clone() for ch in range(3)]
    for i in range(b):
        px, py = torch.round(u[i]), torch.round(v[i])
        inside = (zz[i] > eps) & (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
        zero = torch.zeros_like(px)
        q = torch.where(inside, py, zero).long() * w + torch.where(inside, px, zero).long()   # a clamped address; the tap is discarded
        d = depth[i].reshape(-1)[q]
        wi = torch.ones_like(d) if weight_in is None else weight_in[i].reshape(-1)[q]
        sdf = d - x2[i]
        ok = inside & torch.isfinite(d) & (d > lo) & (d < hi) & torch.isfinite(wi) & (wi > 0) & (sdf >= -tr)
        f = torch.minimum(one, sdf / tr)
        wn = W + wi
        T = torch.where(ok, (T * W + f * wi) / wn, T)
        if C is not None:
            rgb = colors[i].reshape(-1, 3)[q].to(dt)
            C = [torch.where(ok, (C[ch] * W + rgb[..., ch] * wi) / wn, C[ch]) for ch in range(3)]
        W = torch.where(ok, torch.minimum(wn, mw), W)
    return T, W, None if C is None else torch.stack(C, 0)


def _neighbour(t, axis):
    """``t`` shifted so that entry p holds the value of ``p + e_axis`` (axis 0, 1, 2 = x, y, z; the last slice repeats itself)."""
    dim = t.dim() - 1 - axis
    n = t.shape[dim]
    return torch.cat([t.narrow(dim, 1, n - 1), t.narrow(dim, n - 1, 1)], dim)


def crossings_host(tsdf, weight, min_weight=1.):
    """The boolean ``[nz, ny, nx, 3]`` selection of ``um_tsdf_points`` (last index: the axis x, y, z)."""
    mw = _scalar(min_weight, tsdf)
    sel = []
    for a in range(3):
        tn, wn = _neighbour(tsdf, a), _neighbour(weight, a)
        inside = torch.ones_like(tsdf, dtype=torch.bool)
        inside.narrow(2 - a, tsdf.shape[2 - a] - 1, 1).fill_(False)
        sel.append(inside & (weight >= mw) & (wn >= mw) & ((tsdf < 0) != (tn < 0)) & (tsdf.abs() < 1) & (tn.abs() < 1))
    return torch.stack(sel, -1)


def extract_points_host(tsdf, weight, color=None, *, origin, voxel, min_weight=1., capacity=None):
    """``um_tsdf_points`` step by step, in the dtype of ``tsdf``: ``(xyz [N, 3], rgb [N, 3] uint8 or None)`` in ascending
    ``(k, j, i, axis)`` order.  With ``capacity``: ``(xyz, rgb, N)`` -- the rows ``0 .. min(N, capacity) - 1`` that a buffer of
    ``capacity`` rows receives, and the full count."""
    dt = tsdf.dtype
    sel = crossings_host(tsdf, weight, min_weight)
    k, j, i, a = sel.nonzero(as_tuple=True)                                                # ascending (k, j, i, axis)
    if capacity is not None:
        xyz, rgb = extract_points_host(tsdf, weight, color, origin=origin, voxel=voxel, min_weight=min_weight)
        return xyz[:capacity], None if rgb is None else rgb[:capacity], int(k.numel())
    vs = _scalar(voxel, tsdf)
    base = [_scalar(origin[0], tsdf) + i.to(dt) * vs, _scalar(origin[1], tsdf) + j.to(dt) * vs, _scalar(origin[2], tsdf) + k.to(dt) * vs]
    tp = tsdf[k, j, i]
    kn, jn, in_ = k + (a == 2).long(), j + (a == 1).long(), i + (a == 0).long()
    tn = tsdf[kn, jn, in_]
    s = tp / (tp - tn)
    xyz = torch.stack([torch.where(a == ax, base[ax] + s * vs, base[ax]) for ax in range(3)], 1)
    if color is None:
        return xyz, None
    cp, cn = color[:, k, j, i], color[:, kn, jn, in_]
    val = cp + s * (cn - cp)
    rgb = torch.where(val == val, torch.round(val), torch.zeros_like(val)).clamp(0.0, 255.0).to(torch.uint8)
    return xyz, rgb.t().contiguous()


# ------------------------------------------------------------------ host restatement: the mesh
_TET_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_TET_POSITIVE = (True, False, False, True, True, False)
_TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                  # the six edges of a tetrahedron, by corner position


def _tet_corners(tau):
    """The four corner masks of tetrahedron ``tau``: 0, one step, two steps, 7."""
    p = _TET_PERMS[tau]
    return 0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7


def _tet_triangles(pattern, positive):
    """The triangles of a tetrahedron whose corner ``q`` is inside iff bit ``q`` of ``pattern`` is set: a list of triples of edge
    numbers (indices into ``_TET_EDGES``)."""
    ins = [q for q in range(4) if pattern >> q & 1]
    outs = [q for q in range(4) if not pattern >> q & 1]
    edge = lambda q, r: _TET_EDGES.index((min(q, r), max(q, r)))
    if len(ins) == 1:
        a = ins[0]
        tris, rev = [[edge(a, o) for o in outs]], positive == (a % 2 == 1)
    elif len(ins) == 3:
        a = outs[0]
        tris, rev = [[edge(a, i) for i in ins]], not positive == (a % 2 == 1)
    elif len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
        tris, rev = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]], positive == ((a + b) % 2 == 0)
    else:
        return []
    return [t[::-1] for t in tris] if rev else tris


def _shifted(t, m, cells):
    """``t [nz, ny, nx]`` seen from every cell (``cells = True``: ``[nz - 1, ny - 1, nx - 1]``) at the corner mask ``m``."""
    nz, ny, nx = t.shape
    dk, dj, di = m >> 2 & 1, m >> 1 & 1, m & 1
    if cells:
        return t[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
    return t[dk:, dj:, di:]


def mesh_edges_host(tsdf, weight, min_weight=1.):
    """``(active [nz - 1, ny - 1, nx - 1], sel [nz, ny, nx, 7])``, both boolean: the active cells of ``um_tsdf_mesh`` and the owned
    edges that carry a vertex (last index: ``e - 1``)."""
    nz, ny, nx = tsdf.shape
    mw = _scalar(min_weight, tsdf)
    valid = (weight >= mw) & (tsdf.abs() < 1)
    inside = tsdf < 0
    active = _shifted(valid, 0, True).clone()
    for m in range(1, 8):
        active &= _shifted(valid, m, True)
    act = torch.zeros_like(valid)                            # on the voxel grid: False where the voxel is no cell
    act[:nz - 1, :ny - 1, :nx - 1] = active
    sel = []
    for e in range(1, 8):
        has = torch.zeros_like(valid)                        # at least one cell p - s of the edge is active
        for s in range(8):
            if s & e:
                continue
            dk, dj, di = s >> 2 & 1, s >> 1 & 1, s & 1
            has[dk:, dj:, di:] |= act[:nz - dk, :ny - dj, :nx - di]
        cross = torch.zeros_like(valid)
        ek, ej, ei = e >> 2 & 1, e >> 1 & 1, e & 1
        cross[:nz - ek, :ny - ej, :nx - ei] = inside[:nz - ek, :ny - ej, :nx - ei] != _shifted(inside, e, False)
        sel.append(has & cross)
    return active, torch.stack(sel, -1)


def extract_mesh_host(tsdf, weight, color=None, *, origin, voxel, min_weight=1.):
    """``um_tsdf_mesh`` step by step, in the dtype of ``tsdf``: ``(xyz [V, 3], rgb [V, 3] uint8 or None, faces [F, 3] int64)`` -- marching
    tetrahedra on the Kuhn split (the definition: ``include/unimatch_hip.h``), vertices in ascending ``(k, j, i, e)``, faces in ascending
    ``(k, j, i)`` of the cell, then by tetrahedron, then by triangle, counter-clockwise seen from free space.  A corner that stores
    exactly 0 gives ``s`` of 0 or 1 and triangles of zero area; they are KEPT, because the topology stays manifold with them.  In float32
    this is bitwise the device result, in float64 the reference."""
    dt, dev = tsdf.dtype, tsdf.device
    nz, ny, nx = tsdf.shape
    if min(nx, ny, nz) < 2:                                  # no cell
        return (torch.zeros((0, 3), dtype=dt, device=dev), None if color is None else torch.zeros((0, 3), dtype=torch.uint8, device=dev),
                torch.zeros((0, 3), dtype=torch.int64, device=dev))
    active, sel = mesh_edges_host(tsdf, weight, min_weight)
    k, j, i, a = sel.nonzero(as_tuple=True)                                                # ascending (k, j, i, e)
    e = a + 1
    vid = (sel.reshape(-1).cumsum(0) - 1).reshape(sel.shape)                               # the index of every vertex, at its edge
    vs = _scalar(voxel, tsdf)
    base = [_scalar(origin[0], tsdf) + i.to(dt) * vs, _scalar(origin[1], tsdf) + j.to(dt) * vs, _scalar(origin[2], tsdf) + k.to(dt) * vs]
    tp = tsdf[k, j, i]
    kn, jn, in_ = k + (e >> 2 & 1), j + (e >> 1 & 1), i + (e & 1)
    tn = tsdf[kn, jn, in_]
    s = tp / (tp - tn)
    xyz = torch.stack([torch.where((e >> ax & 1) == 1, base[ax] + s * vs, base[ax]) for ax in range(3)], 1)
    rgb = None
    if color is not None:
        cp, cn = color[:, k, j, i], color[:, kn, jn, in_]
        val = cp + s * (cn - cp)
        rgb = torch.where(val == val, torch.round(val), torch.zeros_like(val)).clamp(0.0, 255.0).to(torch.uint8).t().contiguous()
    # faces: the active cells whose corners are not all on one side, in ascending (k, j, i)
    inside = tsdf < 0
    ins = torch.stack([_shifted(inside, m, True) for m in range(8)], -1)                   # [cells, 8]
    ck, cj, ci = (active & ins.any(-1) & ~ins.all(-1)).nonzero(as_tuple=True)
    ins = ins[ck, cj, ci].long()
    rows, keep = [], []
    for tau in range(6):
        v = _tet_corners(tau)
        pattern = sum(ins[:, v[q]] << q for q in range(4))
        edges = torch.stack([vid[ck + (v[q] >> 2 & 1), cj + (v[q] >> 1 & 1), ci + (v[q] & 1), (v[r] ^ v[q]) - 1] for q, r in _TET_EDGES], 1)
        table = [_tet_triangles(p, _TET_POSITIVE[tau]) for p in range(16)]
        count = torch.tensor([len(t) for t in table], device=dev)
        which = torch.tensor([sum(t, []) + [0] * (6 - 3 * len(t)) for t in table], device=dev)       # [16, 6] edge numbers
        rows.append(edges.gather(1, which[pattern]).reshape(-1, 2, 3))
        keep.append(count[pattern][:, None] > torch.arange(2, device=dev))
    faces = torch.stack(rows, 1)[torch.stack(keep, 1)]                                     # [cells, 6, 2, 3] -> cell, tau, triangle
    return xyz, rgb, faces.reshape(-1, 3)


# ------------------------------------------------------------------ the library
def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _origin3(origin):
    return (ctypes.c_float * 3)(*(float(v) for v in origin))


def _check_state(what, tsdf, weight, color):
    for name, t in (('tsdf', tsdf), ('weight', weight), ('color', color)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == tsdf.device):
            raise ValueError(f'{what}: expected {name} as a contiguous CUDA float32 tensor on one device, got {t.dtype} {t.device}')
    if tsdf.dim() != 3 or weight.shape != tsdf.shape or (color is not None and tuple(color.shape) != (3,) + tuple(tsdf.shape)):
        raise ValueError(f'{what}: expected tsdf, weight [nz, ny, nx] and color [3, nz, ny, nx], got {tuple(tsdf.shape)}, '
                         f'{tuple(weight.shape)}, {None if color is None else tuple(color.shape)}')


def integrate_device(tsdf, weight, color, depth, cam_view, weight_in=None, colors=None, *, origin, voxel, trunc, max_weight=64.,
                     min_depth=0., max_depth=float('inf')):
    """``um_tsdf_integrate`` on CUDA tensors: one launch for all views of ``depth [B, H, W]``, the state updated in place.  No
    synchronisation."""
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    _check_state('integrate_device', tsdf, weight, color)
    nz, ny, nx = tsdf.shape
    b, h, w = depth.shape
    for name, t, shape, dtype in (('depth', depth, (b, h, w), torch.float32), ('cam_view', cam_view, (b, 30), torch.float32),
                                  ('weight_in', weight_in, (b, h, w), torch.float32), ('colors', colors, (b, h, w, 3), torch.uint8)):
        if t is not None and not (t.is_cuda and t.device == tsdf.device and t.dtype == dtype and tuple(t.shape) == shape
                                  and t.is_contiguous()):
            raise ValueError(f'integrate_device: expected {name} as a contiguous CUDA {dtype} {shape} on {tsdf.device}, got '
                             f'{t.dtype} {tuple(t.shape)} {t.device}')
    if (colors is None) != (color is None):
        raise ValueError('integrate_device: colors go with a volume that has colour planes, and only with one')
    with torch.cuda.device(tsdf.device):
        _abi.check(lib.um_tsdf_integrate(depth.data_ptr(), cam_view.data_ptr(), _ptr(weight_in), _ptr(colors), tsdf.data_ptr(),
                                         weight.data_ptr(), _ptr(color), nx, ny, nz, _origin3(origin), float(voxel), float(trunc),
                                         float(max_weight), float(min_depth), float(max_depth), b, h, w, _stream()),
                   'um_tsdf_integrate')


def points_device(tsdf, weight, color, *, origin, voxel, min_weight=1., capacity, xyz=None, rgb=None):
    """``um_tsdf_points`` on CUDA tensors: ``(xyz [capacity, 3], rgb [capacity, 3] or None, count)``, ``count`` a one-element int32
    tensor ON THE DEVICE holding the full N; rows ``min(N, capacity)..`` are unwritten.  ``xyz`` / ``rgb``: buffers to write into
    (fresh ones otherwise).  No synchronisation."""
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    _check_state('points_device', tsdf, weight, color)
    nz, ny, nx = tsdf.shape
    capacity, dev = int(capacity), tsdf.device
    with torch.cuda.device(dev):
        xyz = torch.empty((capacity, 3), dtype=torch.float32, device=dev) if xyz is None else xyz
        if color is not None and rgb is None:
            rgb = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
        if tuple(xyz.shape) != (capacity, 3) or xyz.dtype != torch.float32 or not xyz.is_contiguous() or (
                rgb is not None and (tuple(rgb.shape) != (capacity, 3) or rgb.dtype != torch.uint8 or not rgb.is_contiguous())):
            raise ValueError(f'points_device: expected xyz float32 and rgb uint8 as contiguous [{capacity}, 3] buffers')
        count = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = lib.um_tsdf_points_workspace_bytes(nx, ny, nz)
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        _abi.check(lib.um_tsdf_points(tsdf.data_ptr(), weight.data_ptr(), _ptr(color), nx, ny, nz, _origin3(origin), float(voxel),
                                      float(min_weight), xyz.data_ptr(), _ptr(rgb if color is not None else None), count.data_ptr(),
                                      capacity, ws.data_ptr(), nbytes, _stream()), 'um_tsdf_points')
    return xyz, (rgb if color is not None else None), count


def mesh_device(tsdf, weight, color, *, origin, voxel, min_weight=1., vertex_capacity, face_capacity, xyz=None, rgb=None, faces=None):
    """``um_tsdf_mesh`` on CUDA tensors: ``(xyz [vertex_capacity, 3], rgb [vertex_capacity, 3] or None, faces [face_capacity, 3] int32,
    counts)``, ``counts`` a two-element int32 tensor ON THE DEVICE holding the full ``(V, F)``; vertex rows ``min(V, vertex_capacity)..``
    and face rows ``min(F, face_capacity)..`` are unwritten, and a written face row holds the indices into the full vertex list.
    ``xyz`` / ``rgb`` / ``faces``: buffers to write into (fresh ones otherwise).  No synchronisation."""
    lib = _abi.load()                        # raises when the HIP extension is missing: there is no silent fallback
    _check_state('mesh_device', tsdf, weight, color)
    nz, ny, nx = tsdf.shape
    vcap, fcap, dev = int(vertex_capacity), int(face_capacity), tsdf.device
    with torch.cuda.device(dev):
        xyz = torch.empty((vcap, 3), dtype=torch.float32, device=dev) if xyz is None else xyz
        faces = torch.empty((fcap, 3), dtype=torch.int32, device=dev) if faces is None else faces
        if color is not None and rgb is None:
            rgb = torch.empty((vcap, 3), dtype=torch.uint8, device=dev)
        if tuple(xyz.shape) != (vcap, 3) or xyz.dtype != torch.float32 or not xyz.is_contiguous() or (
                rgb is not None and (tuple(rgb.shape) != (vcap, 3) or rgb.dtype != torch.uint8 or not rgb.is_contiguous())):
            raise ValueError(f'mesh_device: expected xyz float32 and rgb uint8 as contiguous [{vcap}, 3] buffers')
        if tuple(faces.shape) != (fcap, 3) or faces.dtype != torch.int32 or not faces.is_contiguous():
            raise ValueError(f'mesh_device: expected faces as a contiguous int32 [{fcap}, 3] buffer')
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        nbytes = lib.um_tsdf_mesh_workspace_bytes(nx, ny, nz)
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        _abi.check(lib.um_tsdf_mesh(tsdf.data_ptr(), weight.data_ptr(), _ptr(color), nx, ny, nz, _origin3(origin), float(voxel),
                                    float(min_weight), xyz.data_ptr(), _ptr(rgb if color is not None else None), faces.data_ptr(),
                                    counts.data_ptr(), vcap, fcap, ws.data_ptr(), nbytes, _stream()), 'um_tsdf_mesh')
    return xyz, (rgb if color is not None else None), faces, counts


# ------------------------------------------------------------------ public interface
class TSDFVolume:
    """A truncated signed distance volume of ``dims = (nx, ny, nz)`` voxels of ``voxel_size`` whose voxel ``(0, 0, 0)`` has its centre at
    ``origin``; ``trunc`` (default: 4 voxels) is the truncation distance, ``max_weight`` the cap of a voxel's accumulated weight (a
    running average over about that many observations).  ``.tsdf``, ``.weight`` ``[nz, ny, nx]`` and ``.color`` ``[3, nz, ny, nx]``
    (``None`` without colour) are float32 tensors on ``device``; CUDA volumes run the HIP kernels, host volumes the restatement."""

    def __init__(self, origin, voxel_size, dims, trunc=None, max_weight=64., with_color=True, device='cuda'):
        self.dims = _check_dims(dims)
        self.origin = tuple(_f32(v) for v in origin)
        if len(self.origin) != 3 or not all(math.isfinite(v) for v in self.origin):
            raise ValueError(f'origin: expected three finite values, got {origin!r}')
        self.voxel_size = _f32(voxel_size)
        self.trunc = _f32(4.0 * self.voxel_size if trunc is None else trunc)
        self.max_weight = _f32(max_weight)
        _check_positive(voxel_size=self.voxel_size, trunc=self.trunc, max_weight=self.max_weight)
        nx, ny, nz = self.dims
        self.device = torch.device(device)
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if with_color else None

    def _grid(self):
        return {'origin': self.origin, 'voxel': self.voxel_size}

    def reset(self):
        """Back to a fresh volume: all zeros."""
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()

    def integrate(self, depth, intrinsics, poses, weight=None, colors=None, min_depth=0., max_depth=float('inf')):
        """Fuse the metric ``depth [B, H, W]`` of B views with ``intrinsics [1 or B, 3, 3]`` and camera-to-world ``poses [B, 4, 4]`` into
        the volume, in ascending order of the views (one launch on the device).  ``weight [B, H, W]``: the per-pixel weight of an
        observation (a confidence, a keep mask; ``None``: 1; non-finite or <= 0: the pixel contributes nothing); ``colors [B, H, W, 3]``
        uint8: required exactly when the volume has colour.  Only pixels with a finite ``min_depth < d < max_depth`` contribute."""
        what = 'TSDFVolume.integrate'
        dev = self.tsdf.device
        b, h, w = _check_views(what, dev, depth, weight, colors)
        if (colors is None) != (self.color is None):
            raise ValueError(f'{what}: colors go with a volume that has colour planes (with_color=True), and only with one')
        geometry._same_device(what, depth, intrinsics=intrinsics, poses=poses)
        k, p = geometry._expand_intrinsics(intrinsics, b, what), geometry._check_poses(poses, b, what)
        depth = depth.float().contiguous()
        weight = None if weight is None else weight.float().contiguous()
        colors = None if colors is None else colors.contiguous()
        kw = dict(self._grid(), trunc=self.trunc, max_weight=self.max_weight, min_depth=min_depth, max_depth=max_depth)
        if dev.type == 'cuda':
            with torch.cuda.device(dev):
                cam_view = geometry._cam_pack(k, p, True)[b:].contiguous()         # the inverse half: world -> camera
                integrate_device(self.tsdf, self.weight, self.color, depth, cam_view, weight, colors, **kw)
            return self
        cam_view = geometry._cam_pack(k, p, True)[b:]
        t, wt, c = integrate_host(self.tsdf, self.weight, self.color, depth, cam_view, weight, colors, **kw)
        self.tsdf.copy_(t)
        self.weight.copy_(wt)
        if c is not None:
            self.color.copy_(c)
        return self

    def extract_points(self, min_weight=1.):
        """``(xyz [N, 3] float32, rgb [N, 3] uint8 or None)``: the zero crossings of the volume along the three axes between voxels of
        weight ``>= min_weight``, in ascending ``(k, j, i, axis)`` order.  On the device: ONE synchronisation (the read of N) after a
        run at a capacity of ``6 (nx ny + ny nz + nx nz)`` rows, and one more run at exactly N only when N exceeds that."""
        if self.tsdf.device.type != 'cuda':
            return extract_points_host(self.tsdf, self.weight, self.color, min_weight=min_weight, **self._grid())
        nx, ny, nz = self.dims
        capacity = 6 * (nx * ny + ny * nz + nx * nz)
        xyz, rgb, count = points_device(self.tsdf, self.weight, self.color, min_weight=min_weight, capacity=capacity, **self._grid())
        n = int(count.item())                                                      # the one synchronisation
        if n > capacity:
            xyz, rgb, _ = points_device(self.tsdf, self.weight, self.color, min_weight=min_weight, capacity=n, **self._grid())
        return xyz[:n], None if rgb is None else rgb[:n]

    def _mesh_capacities(self):
        nx, ny, nz = self.dims
        sheets = 6 * (nx * ny + ny * nz + nx * nz)
        return 4 * sheets, 8 * sheets

    def extract_mesh(self, min_weight=1.):
        """``(xyz [V, 3] float32, rgb [V, 3] uint8 or None, faces [F, 3])``: the triangle mesh of the volume between voxels of weight
        ``>= min_weight`` -- marching tetrahedra on the Kuhn split (:func:`extract_mesh_host`), every face counter-clockwise seen from
        free space; ``faces`` is int32 on the device and int64 on the host.  Zero-area triangles (a corner storing exactly 0) are kept.
        On the device: ONE synchronisation (the read of V and F) after a run at default capacities, and one more run at exactly
        ``(V, F)`` only when either count exceeds its capacity.  The defaults: ``extract_points`` allows ``6 (nx ny + ny nz + nx nz)``
        rows -- six sheets that each project one-to-one onto a side of the box, at one axis crossing per unit of projected area.  A
        sheet with unit normal ``n`` crosses ``|n . d|`` edges of direction ``d`` per unit area, and each axis occurs in four of the
        seven edge directions, so the mesh has at most four vertices per unit of projected area: four times the rows of the points.  A
        surface has ``F = 2 (V - chi) - boundary edges``, so twice as many face rows as vertex rows."""
        if self.tsdf.device.type != 'cuda':
            return extract_mesh_host(self.tsdf, self.weight, self.color, min_weight=min_weight, **self._grid())
        vcap, fcap = self._mesh_capacities()
        xyz, rgb, faces, counts = mesh_device(self.tsdf, self.weight, self.color, min_weight=min_weight, vertex_capacity=vcap,
                                              face_capacity=fcap, **self._grid())
        v, f = (int(n) for n in counts.tolist())                                   # the one synchronisation
        if v > vcap or f > fcap:
            xyz, rgb, faces, _ = mesh_device(self.tsdf, self.weight, self.color, min_weight=min_weight, vertex_capacity=v, face_capacity=f,
                                             **self._grid())                       # a mesh with a face has a vertex: neither is 0
        return xyz[:v], None if rgb is None else rgb[:v], faces[:f]


def volume_bounds(depths, intrinsics, poses, keep=None, min_depth=0., max_depth=float('inf'), stride=4, margin=0.):
    """``(lo, hi)``, two tuples of three floats: the axis-aligned world box of the back-projected pixels of ``depths [T, H, W]`` that
    :func:`unimatch_amd.geometry.back_project_points` selects (``keep``, depth range, every ``stride``-th pixel), grown by ``margin``
    on every side.  Raises ``ValueError`` when no pixel is selected."""
    xyz, _ = geometry.back_project_points(depths, intrinsics, poses, keep=keep, min_depth=min_depth, max_depth=max_depth, stride=stride)
    if xyz.shape[0] == 0:
        raise ValueError('volume_bounds: no pixel with a valid depth is kept: the scene has no extent')
    box = torch.stack([xyz.amin(0), xyz.amax(0)], 0).cpu()
    return tuple(float(v) - float(margin) for v in box[0]), tuple(float(v) + float(margin) for v in box[1])


def _grid_dims(lo, hi, voxel):
    return tuple(int(math.ceil((b - a) / voxel)) + 1 for a, b in zip(lo, hi))


def fuse_depth_sequence_tsdf(depths, intrinsics, poses, colors=None, weight=None, voxel_size=0.04, trunc=None, max_weight=64.,
                             min_weight=1., views_per_launch=8, max_voxels=2 ** 28, min_depth=0., max_depth=float('inf'),
                             bounds_stride=4, mesh=False):
    """The TSDF surface of a posed video: ``dict(xyz [N, 3], rgb [N, 3] or None, volume)``; with ``mesh=True`` the dict also holds
    ``faces [F, 3]`` and ``xyz`` / ``rgb`` are the vertices of the triangle mesh (:meth:`TSDFVolume.extract_mesh`).

    ``depths [T, H, W]`` metric, ``intrinsics [1 or T, 3, 3]``, ``poses [T, 4, 4]`` camera-to-world, ``colors [T, H, W, 3]`` uint8,
    ``weight [T, H, W]`` the per-pixel integration weight (the ``keep`` mask of ``fuse_depth_sequence``, a confidence, ...; <= 0: the
    pixel is not used).  The volume covers :func:`volume_bounds` of the pixels with a positive weight (every ``bounds_stride``-th),
    padded by ``trunc`` (default: 4 voxels); a grid of more than ``max_voxels`` raises a ``ValueError`` that names the voxel size to
    use.  Frames are integrated in chunks of ``views_per_launch`` -- the result does not depend on it -- and the surface is extracted
    between voxels of weight ``>= min_weight``."""
    what = 'fuse_depth_sequence_tsdf'
    if not torch.is_tensor(depths) or depths.dim() != 3:
        raise ValueError(f'{what}: expected depths [T, H, W], got {tuple(getattr(depths, "shape", ()))}')
    t = depths.shape[0]
    step = int(views_per_launch)
    if step < 1:
        raise ValueError(f'{what}: views_per_launch must be >= 1, got {views_per_launch}')
    _check_views(what, depths.device, depths, weight, colors)
    k, p = geometry._expand_intrinsics(intrinsics, t, what), geometry._check_poses(poses, t, what)
    voxel = _f32(voxel_size)
    _check_positive(voxel_size=voxel)
    keep = None if weight is None else (weight > 0).float()
    lo, hi = volume_bounds(depths, k, p, keep=keep, min_depth=min_depth, max_depth=max_depth, stride=bounds_stride)

    def padded(v):                           # the box, padded by the truncation distance that goes with the voxel size v
        pad = _f32(4.0 * v if trunc is None else trunc)
        return pad, tuple(a - pad for a in lo), tuple(b + pad for b in hi)

    pad, origin, top = padded(voxel)
    dims = _grid_dims(origin, top, voxel)
    if dims[0] * dims[1] * dims[2] > int(max_voxels):
        need = voxel
        while math.prod(_grid_dims(*padded(need)[1:], need)) > int(max_voxels):
            need *= 1.02
        raise ValueError(f'{what}: the scene spans {tuple(round(b - a, 3) for a, b in zip(lo, hi))} m: at voxel_size={voxel:g} that is a '
                         f'grid of {dims[0]} x {dims[1]} x {dims[2]} voxels, more than max_voxels={int(max_voxels)}; use '
                         f'voxel_size >= {need * 1.001:.4g}')
    volume = TSDFVolume(origin, voxel, dims, pad, max_weight, colors is not None, depths.device)
    for a in range(0, t, step):
        volume.integrate(depths[a:a + step], k[a:a + step], p[a:a + step], None if weight is None else weight[a:a + step],
                         None if colors is None else colors[a:a + step], min_depth, max_depth)
    if mesh:
        xyz, rgb, faces = volume.extract_mesh(min_weight)
        return {'xyz': xyz, 'rgb': rgb, 'faces': faces, 'volume': volume}
    xyz, rgb = volume.extract_points(min_weight)
    return {'xyz': xyz, 'rgb': rgb, 'volume': volume}
