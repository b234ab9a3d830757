"""Mint ``warp.npz`` from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_warp.py

The reference warps feature maps with ``unimatch.geometry.flow_warp`` (pixel coordinates, bilinear, zeros outside, with the
normalise / un-normalise round trip of ``grid_sample``); ``interp.backward_warp`` applies the same function to images.  Stored per case:
the image (uint8, values 0..255, used as float32 with C = 3 and, its first channel, C = 1), the flow (the seeded smooth flows of
``tests/tracks_util.py`` plus two bands that leave the frame), and the reference's ``flow_warp(image, flow, mask=True)`` for both
channel counts.  ``f64_distance`` is the largest distance of the reference's float32 output from the same function evaluated in
float64 on the same inputs: the test allows 4 x it (float32 summation-order slack).  The file stays far below the size at which
``make_golden_tracks.py`` had to drop a field."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference'))     # a checkout next to this one
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)

from unimatch.geometry import flow_warp  # noqa: E402
from tests.tracks_util import smooth_flows  # noqa: E402

CASES = (('a', 2, 33, 47, 3), ('b', 2, 64, 97, 4))


def case_inputs(b, h, w, seed):
    flow = smooth_flows(b, h, w, seed).clone()
    flow[:, 0, :, w - 6:] += 9.0                  # a band that leaves the frame on the right ...
    flow[:, 1, :4, :] -= 7.0                      # ... and one that leaves it at the top
    g = torch.Generator().manual_seed(seed + 50)
    image = torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8)
    return image, flow.contiguous()


def main():
    out, worst = {}, 0.0
    for tag, b, h, w, seed in CASES:
        image, flow = case_inputs(b, h, w, seed)
        out[f'image_{tag}'] = image.numpy()
        out[f'flow_{tag}'] = flow.numpy()
        for c in (3, 1):
            img = image[:, :c].float()
            warped, mask = flow_warp(img, flow, mask=True)
            exact, mask64 = flow_warp(img.double(), flow.double(), mask=True)
            worst = max(worst, (warped.double() - exact).abs().max().item())
            out[f'warp{c}_{tag}'] = warped.float().numpy()
            if c == 3:
                out[f'mask_{tag}'] = mask.numpy()
                out[f'mask64_agrees_{tag}'] = np.array(bool(torch.equal(mask, mask64)))
    out['f64_distance'] = np.array(worst, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, 'warp.npz'), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})
    print(f'largest |float32 reference - float64 evaluation| = {worst:.3e} (image values 0..255)')
    print('size', os.path.getsize(os.path.join(HERE, 'warp.npz')))


if __name__ == '__main__':
    main()
