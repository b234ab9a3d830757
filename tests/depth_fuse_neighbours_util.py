"""Row tables for the tests of ``um_depth_corr_softmax_multi_rows`` (tests/test_depth_fuse_neighbours_cpu.py, _gpu.py): the
source-major operands of tests/depth_multiview_util.py scattered, in shuffled order, into 1 .. 4 segments between decoy rows of NaN,
with the table that names them; and the table of segment edges of row 10 of tests/test_dispatch_boundaries_gpu.py (``scatter_edges``).
Plain torch on host tensors; deterministic per (shapes, segments, seed)."""
import functools

import torch

from tests import depth_multiview_util as mv

BIG = 2 ** 30                  # a row index far past every table of these tests


def scatter(f0, f1, cam, segments, seed=0, decoys=3):
    """``(segs, cam_table, rows)`` for source-major ``f0``, ``f1`` ``[S, B, L, C]`` and ``cam [S, B, 30]``: ``segs`` is a list of
    ``segments`` tensors ``[n_i, L, C]`` of uneven sizes that together hold the ``2 S B`` operand rows at shuffled places and
    ``decoys + segments`` rows of NaN, ``cam_table [S B + decoys, 30]`` the cam records likewise, ``rows [S, B, 3]`` int32 = f0 row |
    f1 row | cam row.  No row is named twice."""
    s, b, l, c = f0.shape
    g = torch.Generator().manual_seed(4242 + 17 * seed + segments)
    n_tok = 2 * s * b + decoys + segments
    place = torch.randperm(n_tok, generator=g)
    tokens = torch.full((n_tok, l, c), float('nan'), dtype=f0.dtype)
    p0, p1 = place[:s * b].view(s, b), place[s * b:2 * s * b].view(s, b)
    tokens[p0.flatten()] = f0.reshape(s * b, l, c)
    tokens[p1.flatten()] = f1.reshape(s * b, l, c)
    n_cam = s * b + decoys
    pc = torch.randperm(n_cam, generator=g)[:s * b].view(s, b)
    table = torch.full((n_cam, 30), float('nan'), dtype=cam.dtype)
    table[pc.flatten()] = cam.reshape(s * b, 30)
    # uneven cuts, every segment at least one row
    cuts = sorted((1 + torch.randperm(n_tok - 1, generator=g)[:segments - 1]).tolist())
    bounds = [0] + cuts + [n_tok]
    segs = [tokens[lo:hi].contiguous() for lo, hi in zip(bounds[:-1], bounds[1:])]
    rows = torch.stack([p0, p1, pc], -1).to(torch.int32).contiguous()
    return segs, table.contiguous(), rows


def scatter_edges(f0, f1, cam, seed=0, decoys=3):
    """``(segs, cam_table, rows, use)``: four segments of sizes 1, n, 1, m whose FIRST and LAST rows are all operands that ``rows`` names
    (rows 0 | 1, n | n + 1 | n + 2, total - 1 of the concatenation), ``decoys`` rows of NaN elsewhere.  Source 1 is off in the last
    sample: its f0 row is ``total``, the first index past the end, and the entry before it (source 1, the sample before) has f0 row
    ``total - 1``, the last valid one.  ``use [S, B]`` uint8 is the mask the contiguous launch needs for the same sweep.  The operands of
    the off source are in no segment.  Needs ``2 (S B - 1) >= 6`` operand rows and ``B >= 2``."""
    s, b, l, c = f0.shape
    assert b >= 2 and s >= 2 and 2 * (s * b - 1) >= 6
    g = torch.Generator().manual_seed(5151 + 17 * seed)
    use = torch.ones(s, b, dtype=torch.uint8)
    use[1, b - 1] = 0
    on = [(i, j) for i in range(s) for j in range(b) if use[i, j]]
    total = 2 * len(on) + decoys
    n = (total - 2) // 2
    sizes = [1, n, 1, total - 2 - n]
    edges = [0, 1, n, n + 1, n + 2, total - 1]
    assert len(set(edges)) == 6 and min(sizes) >= 1
    # operand k of 2 len(on): f0 of on[k // 2] (even k) or its f1 (odd k); the f0 of (1, b - 2) takes the last row, five others the
    # remaining edges, the rest any other row
    last = 2 * on.index((1, b - 2))
    order = [k for k in torch.randperm(2 * len(on), generator=g).tolist() if k != last]
    inner = [r for r in torch.randperm(total, generator=g).tolist() if r not in edges]
    place = {last: total - 1}
    place.update(zip(order[:5], edges[:5]))
    place.update(zip(order[5:], inner))
    tokens = torch.full((total, l, c), float('nan'), dtype=f0.dtype)
    n_cam = s * b + decoys
    pc = torch.randperm(n_cam, generator=g)[:s * b].view(s, b)
    table = torch.full((n_cam, 30), float('nan'), dtype=cam.dtype)
    rows = torch.zeros(s, b, 3, dtype=torch.int32)
    for k, (i, j) in enumerate(on):
        tokens[place[2 * k]], tokens[place[2 * k + 1]] = f0[i, j], f1[i, j]
        table[pc[i, j]] = cam[i, j]
        rows[i, j] = torch.tensor([place[2 * k], place[2 * k + 1], int(pc[i, j])], dtype=torch.int32)
    rows[1, b - 1] = torch.tensor([total, 0, int(pc[0, 0])], dtype=torch.int32)            # ONE bad index: the first row past the end
    bounds = [0, 1, n + 1, n + 2, total]
    segs = [tokens[lo:hi].contiguous() for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert [t.shape[0] for t in segs] == sizes
    return segs, table.contiguous(), rows.contiguous(), use


@functools.lru_cache(maxsize=None)
def edges_case(case):
    """``scatter_edges`` of a case of tests/depth_multiview_util.py with the float64 reference of the same sweep (source 1 off in the
    last sample): ``(segs, cam_table, rows, use, reference)``, computed once, shared, never modified."""
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows, use = scatter_edges(f0, f1, cam, seed=len(moves) + d)
    return segs, table, rows, use, mv.reference_of(f0, f1, h, w, cam, cand, use)


def switch_off(rows, use, total_rows, cam_rows, shift=0):
    """``rows`` with every source that ``use [S, B]`` switches off given ONE bad index, a different kind from one off source to the next
    (``shift`` rotates the kinds): a negative f0 row, an f1 row == total_rows, a cam row == cam_rows, a negative cam row, an f0 row far
    past the end, the most negative f1 row, all three -1."""
    rows = rows.clone()
    kinds = [(0, -1), (1, total_rows), (2, cam_rows), (2, -5), (0, BIG), (1, -2 ** 31), (None, -1)]
    n = shift
    for s in range(rows.shape[0]):
        for b in range(rows.shape[1]):
            if not bool(use[s, b]):
                col, val = kinds[n % len(kinds)]
                if col is None:
                    rows[s, b] = val
                else:
                    rows[s, b, col] = val
                n += 1
    return rows
