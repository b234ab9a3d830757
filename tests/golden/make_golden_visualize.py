"""Mint ``visualize.npz`` from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_visualize.py

Pins the two visualisation functions the reference's ``inference_stereo`` / ``inference_depth`` apply to a prediction:
``utils.visualization.vis_disparity`` and ``viz_depth_tensor``.  That module imports ``cv2`` and ``torchvision``; where they are
not installed, empty stand-in modules are registered before the import, with ``cv2.applyColorMap`` as the identity, so that
``vis_disparity`` returns the INDEX image (what is pinned: the table itself is OpenCV's).  ``viz_depth_tensor`` needs matplotlib and
returns colours.  Inputs are seeded, smooth plus a little noise: depths in 0.5 .. 10 (the function is given ``1 / depth``, as the
reference calls it), disparities in 0 .. 192.  The NumPy and matplotlib versions are stored with the results: NumPy's percentile
arithmetic depends on its version.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', '/root/reference')
sys.path.insert(0, REFERENCE)

SIZES = ((3, 37, 53), (1, 64, 96), (2, 48, 64), (1, 120, 160))


def stand_ins():
    try:
        import cv2  # noqa: F401
    except ImportError:
        cv2 = types.ModuleType('cv2')
        cv2.COLORMAP_INFERNO = 14
        cv2.applyColorMap = lambda img, cmap: img
        sys.modules['cv2'] = cv2
    else:
        sys.modules['cv2'].applyColorMap = lambda img, cmap: img
    try:
        import torchvision.utils  # noqa: F401
    except ImportError:
        tv, tvu = types.ModuleType('torchvision'), types.ModuleType('torchvision.utils')
        tv.utils = tvu
        sys.modules['torchvision'], sys.modules['torchvision.utils'] = tv, tvu


def smooth(seed, b, h, w, lo, hi, noise):
    """``[b, h, w]`` float32 in ``[lo, hi]``: a bilinearly upsampled coarse random field plus ``noise`` of the range of white noise."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b, 1, max(2, h // 8), max(2, w // 8), generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True)[:, 0]
    field = (field + noise * torch.rand(b, h, w, generator=g)) / (1 + noise)
    return (lo + (hi - lo) * field).float().contiguous()


def inputs():
    out = {}
    for i, (b, h, w) in enumerate(SIZES):
        out[f'disp_in_{i}'] = smooth(100 + i, b, h, w, 0.0, 192.0, 0.02).numpy()
        out[f'depth_in_{i}'] = smooth(200 + i, b, h, w, 0.5, 10.0, 0.02).numpy()
    return out


def main():
    stand_ins()
    import matplotlib
    from utils.visualization import vis_disparity, viz_depth_tensor
    out = {'numpy_version': np.array(np.__version__), 'matplotlib_version': np.array(matplotlib.__version__)}
    out.update(inputs())
    for i in range(len(SIZES)):
        disp, depth = out[f'disp_in_{i}'], out[f'depth_in_{i}']
        out[f'disp_idx_{i}'] = np.stack([vis_disparity(d.copy()) for d in disp], 0)
        out[f'depth_rgb_{i}'] = np.stack([viz_depth_tensor(1. / torch.from_numpy(d.copy()), return_numpy=True) for d in depth], 0)
        assert out[f'disp_idx_{i}'].dtype == np.uint8 and out[f'depth_rgb_{i}'].dtype == np.uint8
    np.savez_compressed(os.path.join(HERE, 'visualize.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
