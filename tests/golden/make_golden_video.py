"""Mint ``video.npz`` from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_video.py

Pins the two post-processing functions the reference's ``inference_flow`` applies to every predicted flow:
``unimatch.geometry.forward_backward_consistency_check`` (torch, CPU) and ``utils.flow_viz.flow_to_image`` (NumPy; it writes into
its input, so it gets copies).  Inputs are seeded and chosen to reach every branch: flows pointing out of frame, an all-zero flow
(maximum radius 0), unknown flow above 1e7 and +-inf, a NaN (which turns the image's ``max(-1, np.max(rad))`` into -1), radii just
below and above 1 after the normalisation, and one batch whose images have maxima five orders of magnitude apart.  The NumPy version
the colours were produced with is stored with them (its promotion rules decide which steps are float64).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', '/root/reference')
sys.path.insert(0, REFERENCE)

from unimatch.geometry import forward_backward_consistency_check  # noqa: E402
from utils.flow_viz import flow_to_image  # noqa: E402


def smooth_flow(seed, b, h, w, scale):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(b, 2, max(2, h // 8), max(2, w // 8), generator=g)
    return (torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True) * scale).float()


def backward_of(fwd, seed, bad_fraction=0.15):
    """A backward flow that mostly cancels the forward one (a near-zero residual) with inconsistent patches."""
    g = torch.Generator().manual_seed(seed)
    b, _, h, w = fwd.shape
    bwd = -fwd + 0.05 * torch.randn(fwd.shape, generator=g)
    bad = torch.rand(b, 1, h, w, generator=g) < bad_fraction
    return torch.where(bad, bwd + 6.0 * torch.randn(fwd.shape, generator=g), bwd).float().contiguous()


def ring_flow(seed, h, w, radius):
    """Every pixel at |flow| ~= radius (relative spread 1e-6): after the normalisation some land just above 1, some just below."""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(h, w, generator=g, dtype=torch.float64) * 2 * np.pi
    r = radius * (1 + 1e-6 * torch.randn(h, w, generator=g, dtype=torch.float64))
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], 0).float()


def colour(flows):
    """flow_to_image of each image of [B, 2, H, W] on a fresh [H, W, 2] copy."""
    return np.stack([flow_to_image(np.ascontiguousarray(f.permute(1, 2, 0).numpy().copy())) for f in flows], 0)


def main():
    out = {'numpy_version': np.array(np.__version__)}
    # occlusion: one batch of three odd-sized pairs (out-of-frame flows near the borders), one 96 x 128 pair
    drift = torch.tensor([3.2, -1.7]).view(1, 2, 1, 1)             # a translation plus a slowly varying part
    fwd_a = drift + smooth_flow(11, 3, 37, 53, 0.2)
    fwd_a[:, 0, :, :4] -= 12.0                                      # leaves the frame on the left ...
    fwd_a[:, 1, -3:, :] += 9.0                                      # ... and at the bottom
    bwd_a = backward_of(fwd_a, 12)
    fwd_b = 4 * drift + smooth_flow(13, 1, 96, 128, 0.3)
    bwd_b = backward_of(fwd_b, 14)
    for tag, f, b in (('a', fwd_a, bwd_a), ('b', fwd_b, bwd_b)):
        occ_f, occ_b = forward_backward_consistency_check(f.clone(), b.clone())
        out[f'occ_fwd_in_{tag}'], out[f'occ_bwd_in_{tag}'] = f.numpy(), b.numpy()
        out[f'occ_fwd_{tag}'], out[f'occ_bwd_{tag}'] = occ_f.numpy(), occ_b.numpy()
    # colouring: five 37 x 53 images with very different content and maxima, and a 96 x 128 flow
    col = torch.zeros(5, 2, 37, 53)
    col[0] = smooth_flow(16, 1, 37, 53, 60.0)[0]
    col[0, 0, 5, 7] = 3e7                                           # unknown flow
    col[0, 1, 20, 30] = -2e7
    col[0, 0, 30, 40] = float('inf')
    # col[1] stays exactly zero: maximum radius 0
    col[2] = smooth_flow(17, 1, 37, 53, 1e-3)[0]
    col[2, 1, 10, 10] = float('nan')                                # a NaN: max(-1, np.max(rad)) = -1 for this image
    col[2, 0, 11, 12] = 5e7                                         # an unknown pixel next to it
    col[3] = ring_flow(15, 37, 53, 3.7)
    col[4] = ring_flow(19, 37, 53, 1.0)                             # with a NaN the divisor is -1 + eps: radii straddle 1
    col[4, 0, 0, 0] = float('nan')
    out['rgb_in_a'] = col.numpy()
    out['rgb_a'] = colour(col)
    col_b = fwd_b + smooth_flow(18, 1, 96, 128, 8.0)
    out['rgb_in_b'] = col_b.numpy()
    out['rgb_b'] = colour(col_b)
    np.savez_compressed(os.path.join(HERE, 'video.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
