"""Row tables for the tests of ``um_depth_corr_softmax_multi_rows`` (tests/test_depth_fuse_neighbours_cpu.py, _gpu.py): the
source-major operands of tests/depth_multiview_util.py scattered, in shuffled order, into 1 .. 4 segments between decoy rows of NaN,
with the table that names them.  Plain torch on host tensors; deterministic per (shapes, segments, seed)."""
import torch

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
