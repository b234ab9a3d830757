"""Mint ``geometry.npz`` from the REAL reference (runs only where the reference checkout exists):

    UNIMATCH_REFERENCE=<checkout> python tests/golden/make_golden_geometry.py

Pins the reference functions that the consistency checks and the point clouds restate (``unimatch/geometry.py``):

  * ``back_project``, ``camera_transform`` and ``reproject_coords(..., return_mask=True)`` on two seeded plane scenes (float32, CPU):
    the camera-space points of the reference view, the same points in the source view, their pixel coordinates there and the
    in-view mask;
  * ``forward_backward_consistency_check`` on the flows ``(-dL, 0)`` / ``(dR, 0)`` of two seeded disparity pairs, one of which has a
    band displaced far out of frame.

Only inputs and recorded results are stored (masks as uint8).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE')
if not REFERENCE or not os.path.isdir(REFERENCE):
    raise SystemExit('set UNIMATCH_REFERENCE to a checkout of the reference')
sys.path.insert(0, REFERENCE)
sys.path.insert(1, ROOT)

from unimatch.geometry import back_project, camera_transform, forward_backward_consistency_check, reproject_coords  # noqa: E402

from tests.geometry_util import disparity_flows, disparity_pair, plane_pair  # noqa: E402


def main():
    out = {}
    for tag, (seed, b, h, w) in (('a', (31, 1, 33, 47)), ('b', (32, 1, 24, 40))):
        depth, _, k, pose = plane_pair(seed, b, h, w, invalid=False)
        points = back_project(depth, k)
        moved = camera_transform(points, extrinsics_rel=pose)
        coords, mask = reproject_coords(depth, k, extrinsics_rel=pose, return_mask=True)
        out[f'depth_{tag}'], out[f'k_{tag}'], out[f'pose_{tag}'] = depth.numpy(), k.numpy(), pose.numpy()
        out[f'points_{tag}'], out[f'moved_{tag}'] = points.numpy(), moved.numpy()
        out[f'coords_{tag}'], out[f'mask_{tag}'] = coords.numpy(), mask.numpy().astype(np.uint8)
    for tag, (seed, b, h, w, band) in (('a', (41, 2, 33, 47, False)), ('b', (42, 1, 24, 64, True))):
        dl, dr = disparity_pair(seed, b, h, w, band=band)
        occ_l, occ_r = forward_backward_consistency_check(*disparity_flows(dl, dr))
        out[f'disp_left_{tag}'], out[f'disp_right_{tag}'] = dl.numpy(), dr.numpy()
        out[f'occ_left_{tag}'], out[f'occ_right_{tag}'] = occ_l.numpy().astype(np.uint8), occ_r.numpy().astype(np.uint8)
    path = os.path.join(HERE, 'geometry.npz')
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
