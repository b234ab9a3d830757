"""Shared helpers of the TSDF fusion tests: an analytic scene rendered in float64, the three volume cases, the fp64 evaluation of the
definition and the rule that tells decided voxels from undecided ones.

Scene: the plane ``n . X = 2`` with ``n = (0.1, -0.2, 1) / |n|`` behind the sphere of radius 0.35 around (0.1, 0, 1.5); the depth of a
pixel is the camera-z of the nearer hit.  ``fx = 0.9 W``, ``fy = 0.95 W``, principal point ``((W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2)``;
seeded camera-to-world poses with rotations within +-0.15 rad per axis and translations within +-0.2.  The volume starts at
(-0.9, -0.7, 0.9), truncates at 4 voxels and takes depths in 0.1 < d < 10.  The cases are ragged against 64-wide waves and 256-thread
workgroups (nx = 37, 40, 48)."""
import functools
import math

import numpy as np
import torch

from unimatch_amd import fusion
from unimatch_amd.geometry import cam_pack_host

PLANE_N = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])
PLANE_D = 2.0
SPHERE_C, SPHERE_R = np.array([0.1, 0.0, 1.5]), 0.35
ORIGIN = (-0.9, -0.7, 0.9)
MIN_DEPTH, MAX_DEPTH = 0.1, 10.0
#        voxel, views, (H, W), (nx, ny, nz)
CASES = {1: (0.05, 1, (33, 47), (37, 29, 23)),
         2: (0.05, 3, (24, 40), (40, 21, 33)),
         3: (0.04, 4, (48, 64), (48, 40, 36))}


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    mx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    my = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    mz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return mz @ my @ mx


def cameras(views, h, w, seed):
    """``(intrinsics [1, 3, 3], poses [views, 4, 4])`` float32 tensors (the values every evaluation starts from)."""
    rng = np.random.default_rng(seed)
    k = np.array([[0.9 * w, 0, (w - 1) / 2 + 0.3], [0, 0.95 * w, (h - 1) / 2 - 0.2], [0, 0, 1]])
    poses = np.tile(np.eye(4), (views, 1, 1))
    for p in poses:
        p[:3, :3] = _rotation(*rng.uniform(-0.15, 0.15, 3))
        p[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return torch.from_numpy(k[None]).float(), torch.from_numpy(poses).float()


def render(k, poses, h, w):
    """The analytic depth ``[views, H, W]`` in float64 of the float32 cameras: the camera-z of the nearer of plane and sphere."""
    kinv = np.linalg.inv(k[0].double().numpy())
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    rays = np.stack([gx, gy, np.ones_like(gx)], -1) @ kinv.T                         # camera rays with z = 1: the parameter IS the depth
    out = []
    for p in poses.double().numpy():
        dirs, t = rays @ p[:3, :3].T, p[:3, 3]
        plane = (PLANE_D - PLANE_N @ t) / (dirs @ PLANE_N)
        oc = t - SPHERE_C
        a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        out.append(np.minimum(np.where(plane > 0, plane, np.inf), np.where(sphere > 0, sphere, np.inf)))
    return torch.from_numpy(np.stack(out, 0))


def surface_distance(xyz):
    """Distance of world points ``[N, 3]`` (float64 array) to the nearer analytic surface."""
    return np.minimum(np.abs(xyz @ PLANE_N - PLANE_D), np.abs(np.linalg.norm(xyz - SPHERE_C, axis=1) - SPHERE_R))


class Case:
    """One volume case: the float32 inputs every evaluation shares, the two host evaluations (float32, float64) of the definition and
    the decided-voxel rule with its margins.  Built once per case (:func:`case`) and never modified."""

    def __init__(self, number):
        self.voxel, self.views, (self.h, self.w), self.dims = CASES[number]
        self.trunc = 4 * self.voxel
        b, h, w = self.views, self.h, self.w
        self.k, self.poses = cameras(b, h, w, 100 + number)
        self.depth = render(self.k, self.poses, h, w).float()
        g = torch.Generator().manual_seed(200 + number)
        self.colors = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
        # weights whose sums are exact in both precisions: the accumulated weight of a decided voxel is then EQUAL, not close
        self.weight_in = torch.tensor([0.0, 0.5, 1.0, 1.0, 2.0])[torch.randint(0, 5, (b, h, w), generator=g)]
        self.cam_view = cam_pack_host(self.k.expand(b, 3, 3).contiguous(), self.poses, True)[b:].contiguous()
        self.grid = dict(origin=ORIGIN, voxel=self.voxel)
        self.kw = dict(self.grid, trunc=self.trunc, max_weight=64., min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
        nx, ny, nz = self.dims
        self.host32 = self.evaluate(torch.float32)
        self.host64 = self.evaluate(torch.float64)
        self.plain64 = self.evaluate(torch.float64, weighted=False)                 # weights = view counts: min_weight = B is meaningful
        # ---- decided voxels: the rule of the issue, from the two host evaluations only
        x2, zz, u64, v64 = fusion.voxel_projection_host(self.cam_view, ORIGIN, self.voxel, self.dims, torch.float64)
        _, _, u32, v32 = fusion.voxel_projection_host(self.cam_view, ORIGIN, self.voxel, self.dims, torch.float32)
        self.e = 4 * max(float((u32.double() - u64).abs().max()), float((v32.double() - v64).abs().max()))
        near_half = lambda t: ((t - torch.floor(t)) - 0.5).abs() < self.e
        px, py = torch.round(u64).clamp(0, w - 1).long(), torch.round(v64).clamp(0, h - 1).long()
        d = torch.stack([self.depth[i].double().reshape(-1)[py[i] * w + px[i]] for i in range(b)], 0)
        sdf = d - x2
        undecided = near_half(u64) | near_half(v64) | ((sdf + np.float32(self.trunc)).abs() < 1e-5) | ((zz - np.float32(1e-3)).abs() < 1e-5)
        self.decided = ~undecided.any(0)
        self.undecided_share = 1.0 - float(self.decided.double().mean())
        self.updated_share = float((self.host64[1] > 0).double().mean())
        self.tsdf_margin = 4 * float((self.host32[0].double() - self.host64[0])[self.decided].abs().max())

    def volume(self, dtype, color=True):
        nx, ny, nz = self.dims
        return torch.zeros(nz, ny, nx, dtype=dtype), torch.zeros(nz, ny, nx, dtype=dtype), (torch.zeros(3, nz, ny, nx, dtype=dtype) if color else None)

    def evaluate(self, dtype, weighted=True, color=True):
        """The definition evaluated on the host in ``dtype``: ``(tsdf, weight, color)``."""
        t, wt, c = self.volume(dtype, color)
        return fusion.integrate_host(t, wt, c, self.depth, self.cam_view, self.weight_in if weighted else None,
                                     self.colors if color else None, **self.kw)


@functools.lru_cache(maxsize=None)
def case(number):
    return Case(number)


def points_loop(tsdf, weight, color, origin, voxel, min_weight, centre=np.float64):
    """``um_tsdf_points`` as a direct triple loop over float64 copies of the stored values: ``(xyz [N, 3] float64, rgb [N, 3] uint8 or
    None, [(k, j, i, axis)])`` in the order of the definition.  ``centre=np.float32``: the voxel centre is the float32 value the
    definition gives it (``ox + (float)i voxel``, product and sum rounded on their own) and only what follows -- the subtraction, the
    division, the product and the sum of the crossing -- is evaluated in float64."""
    t, wt = tsdf.double().numpy(), weight.double().numpy()
    c = None if color is None else color.double().numpy()
    nz, ny, nx = t.shape
    o, vs = [float(np.float32(v)) for v in origin], float(np.float32(voxel))
    at = lambda a, n: float(centre(o[a]) + centre(n) * centre(vs))
    xyz, rgb, where = [], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                tp = t[k, j, i]
                if not (wt[k, j, i] >= min_weight and abs(tp) < 1):
                    continue
                for a, (dk, dj, di) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
                    kk, jj, ii = k + dk, j + dj, i + di
                    if kk >= nz or jj >= ny or ii >= nx:
                        continue
                    tn = t[kk, jj, ii]
                    if not (wt[kk, jj, ii] >= min_weight and (tp < 0) != (tn < 0) and abs(tn) < 1):
                        continue
                    s = tp / (tp - tn)
                    p = [at(0, i), at(1, j), at(2, k)]
                    p[a] += s * vs
                    xyz.append(p)
                    where.append((k, j, i, a))
                    if c is not None:
                        rgb.append(np.clip(np.rint(c[:, k, j, i] + s * (c[:, kk, jj, ii] - c[:, k, j, i])), 0, 255))
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return xyz, (None if c is None else np.asarray(rgb).reshape(-1, 3).astype(np.uint8)), where
