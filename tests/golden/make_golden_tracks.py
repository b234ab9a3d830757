"""Mint ``tracks.npz`` from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_tracks.py

The reference has no tracker, but it defines what a chain of flows must agree with: ``unimatch.geometry.flow_warp`` (pixel
coordinates, bilinear, zeros outside) and ``forward_backward_consistency_check``.  Composing flows with its own ``flow_warp``,

    F(0 -> t+1) = F(0 -> t) + flow_warp(F(t -> t+1), F(0 -> t)),

is the dense chain.  Stored per case (float32 only): the seeded smooth forward flows, the reference's forward occlusion masks of
them against backward flows that mostly cancel them, and the reference's composition.  The inputs are those of
``tests/tracks_util.py``.  Smooth float32 fields hardly compress, so the backward flows are stored for the small case only (the
large case's would take the file past the repository's limit for a committed file); the masks of both cases are."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference'))     # a checkout next to this one
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)

from unimatch.geometry import flow_warp, forward_backward_consistency_check  # noqa: E402
from tests.tracks_util import smooth_flows  # noqa: E402

CASES = (('a', 8, 33, 47, 3), ('b', 6, 64, 97, 4))


def main():
    out = {}
    for tag, P, h, w, seed in CASES:
        fwd = smooth_flows(P, h, w, seed)
        bwd = (-flow_warp(fwd, -fwd) + smooth_flows(P, h, w, seed + 100, amp=0.35, drift=(0, 0))).float()
        occ = forward_backward_consistency_check(fwd.clone(), bwd.clone())[0]
        acc = fwd[0:1].clone()
        comp = [acc]
        for t in range(1, P):
            acc = acc + flow_warp(fwd[t:t + 1], acc)
            comp.append(acc)
        out[f'fwd_{tag}'] = fwd.numpy()
        if tag == 'a':
            out[f'bwd_{tag}'] = bwd.numpy()
        out[f'occ_fwd_{tag}'] = occ.float().numpy()
        out[f'comp_{tag}'] = torch.cat(comp, 0).float().numpy()
    np.savez_compressed(os.path.join(HERE, 'tracks.npz'), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == '__main__':
    main()
