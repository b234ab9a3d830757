"""Shared helpers of the TSDF mesh tests: the analytic sphere volume, a direct triple-loop evaluation of the marching-tetrahedra
definition in float64 (written from the definition's text at ``um_tsdf_mesh`` in include/unimatch_hip.h, with a dict keyed by edge --
not from ``fusion.extract_mesh_host`` and its ranks) and the topology figures of a face list."""
import functools

import numpy as np
import torch

SPHERE_DIMS = (37, 29, 23)
SPHERE_VOXEL = 0.05
SPHERE_ORIGIN = (0.0, 0.0, 0.0)
SPHERE_CENTRE = np.array([17.3, 13.6, 11.2]) * SPHERE_VOXEL
SPHERE_RADIUS = 8.4 * SPHERE_VOXEL
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
POSITIVE = (True, False, False, True, True, False)


def sphere_volume(dims=SPHERE_DIMS, voxel=SPHERE_VOXEL, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS, seed=None):
    """``(tsdf, weight, color)`` float64 tensors, written directly: ``clamp((|X - c| - r) / trunc, -1, 1)`` with a truncation of 4
    voxels, weight 1 everywhere; ``seed``: random colour planes in 0..255 (``None``: no colour)."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    x = np.stack([i, j, k], -1) * voxel
    t = np.clip((np.linalg.norm(x - centre, axis=-1) - radius) / (4 * voxel), -1, 1)
    color = None if seed is None else torch.from_numpy(np.random.default_rng(seed).uniform(0, 255, (3, nz, ny, nx)))
    return torch.from_numpy(t), torch.ones(nz, ny, nx, dtype=torch.float64), color


@functools.lru_cache(maxsize=None)
def sphere():
    """The sphere volume of the issue with colours, float64; shared, never modified."""
    return sphere_volume(seed=3)


def step(p, m):
    """Voxel ``p = (i, j, k)`` moved by the mask ``m`` (bit 0 = +x, bit 1 = +y, bit 2 = +z)."""
    return p[0] + (m & 1), p[1] + (m >> 1 & 1), p[2] + (m >> 2 & 1)


def mesh_loop(tsdf, weight, color, origin, voxel, min_weight, centre=np.float64):
    """The definition as a direct triple loop over float64 copies of the stored values: ``(xyz [V, 3] float64, rgb [V, 3] uint8 or
    None, faces [F, 3] int64, [(k, j, i, e)] per vertex, [(k, j, i)] the cell of every face)``.  ``centre=np.float32``: the voxel centre
    is the float32 value the definition gives it and everything after it is evaluated in float64."""
    t, wt = tsdf.double().numpy(), weight.double().numpy()
    c = None if color is None else color.double().numpy()
    nz, ny, nx = t.shape
    o, vs = [float(np.float32(v)) for v in origin], float(np.float32(voxel))
    at = lambda a, n: float(centre(o[a]) + centre(n) * centre(vs))
    val = lambda p: t[p[2], p[1], p[0]]
    inside = lambda p: bool(val(p) < 0)
    valid = lambda p: bool(wt[p[2], p[1], p[0]] >= min_weight and abs(val(p)) < 1)

    def active(cell):
        if min(cell) < 0 or cell[0] >= nx - 1 or cell[1] >= ny - 1 or cell[2] >= nz - 1:
            return False
        return all(valid(step(cell, m)) for m in range(8))

    # vertices: ascending (k, j, i, e); an edge carries one when its ends differ in sign and one of its cells is active
    index, where, xyz, rgb = {}, [], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                p = (i, j, k)
                for e in range(1, 8):
                    n = step(p, e)
                    if n[0] >= nx or n[1] >= ny or n[2] >= nz or inside(p) == inside(n):
                        continue
                    free = [b for b in range(3) if not e >> b & 1]
                    cells = []
                    for sub in range(1 << len(free)):
                        s = sum(1 << free[b] for b in range(len(free)) if sub >> b & 1)
                        cells.append((i - (s & 1), j - (s >> 1 & 1), k - (s >> 2 & 1)))
                    if not any(active(cell) for cell in cells):
                        continue
                    tp, tn = val(p), val(n)
                    s = tp / (tp - tn)
                    index[(p, e)] = len(where)
                    where.append((k, j, i, e))
                    base = [at(0, i), at(1, j), at(2, k)]
                    xyz.append([base[a] + s * vs if e >> a & 1 else base[a] for a in range(3)])
                    if c is not None:
                        cp, cn = c[:, k, j, i], c[:, n[2], n[1], n[0]]
                        v = cp + s * (cn - cp)
                        rgb.append(np.clip(np.where(np.isnan(v), 0.0, np.rint(v)), 0, 255))
    # faces: ascending (k, j, i) of the cell, then the tetrahedron, then the triangle
    faces, owner = [], []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                cell = (i, j, k)
                if not active(cell):
                    continue
                for tau, (pi, positive) in enumerate(zip(PERMS, POSITIVE)):
                    v = [0, 1 << pi[0], (1 << pi[0]) | (1 << pi[1]), 7]

                    def E(q, r):
                        q, r = min(q, r), max(q, r)
                        return index[(step(cell, v[q]), v[r] ^ v[q])]

                    ins = [q for q in range(4) if inside(step(cell, v[q]))]
                    outs = [q for q in range(4) if q not in ins]
                    if len(ins) == 1:
                        a = ins[0]
                        tris, rev = [(E(a, outs[0]), E(a, outs[1]), E(a, outs[2]))], positive == (a % 2 == 1)
                    elif len(ins) == 3:
                        a = outs[0]
                        tris, rev = [(E(a, ins[0]), E(a, ins[1]), E(a, ins[2]))], not (positive == (a % 2 == 1))
                    elif len(ins) == 2:
                        (a, b), (cc, d) = ins, outs
                        q = (E(a, cc), E(a, d), E(b, d), E(b, cc))
                        tris, rev = [(q[0], q[1], q[2]), (q[0], q[2], q[3])], positive == ((a + b) % 2 == 0)
                    else:
                        continue
                    faces += [tri[::-1] if rev else tri for tri in tris]
                    owner += [(k, j, i)] * len(tris)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return (xyz, None if c is None else np.asarray(rgb).reshape(-1, 3).astype(np.uint8), np.asarray(faces, np.int64).reshape(-1, 3), where,
            owner)


def topology(faces):
    """``(faces per undirected edge: the set of counts, the largest number of repeats of a directed edge, E)`` of a face list."""
    f = np.asarray(faces, np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, repeats = np.unique(directed, axis=0, return_counts=True)
    edges, per_edge = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    return set(per_edge.tolist()), int(repeats.max()) if len(repeats) else 0, len(edges)


def assert_closed_outward(xyz, faces, centre):
    """The properties of a closed sphere-like surface: two faces per edge, each directed edge once, Euler characteristic 2, every
    normal pointing away from ``centre``, no unreferenced vertex."""
    v, f = np.asarray(xyz, np.float64), np.asarray(faces, np.int64)
    per_edge, repeats, edges = topology(f)
    assert per_edge == {2} and repeats == 1
    assert len(v) - edges + len(f) == 2
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert (np.einsum('ij,ij->i', np.cross(b - a, c - a), (a + b + c) / 3 - centre) > 0).all()
    assert len(np.unique(f)) == len(v)
