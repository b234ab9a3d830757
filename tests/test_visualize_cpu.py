"""CPU tests of ``unimatch_amd.visualize``: the host recipe against fixtures minted from the reference's ``vis_disparity`` and
``viz_depth_tensor`` (tests/golden/visualize.npz), the tables, the percentile's definition, and the C ABI's argument checks.

Disparity indices must be the reference's exactly.  The inverse-depth image may differ from the reference's by one table index on
at most 1e-3 of an image's pixels: NumPy's percentile arithmetic depends on its version (NumPy 2 carries the quantile in float32),
so the reference itself moves ``vmax`` by a few ulps between installations, while the recipe here is one fixed choice.  That cap is a
condition on the fixtures, not a measurement (with NumPy 2.2.6 and matplotlib 3.10.8 the worst fixture image has 3.3e-4)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from unimatch_amd import _abi, visualize
from tests.visualize_util import GROUPS, load_golden, plasma_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables():
    plasma, inferno = visualize.colormap('plasma'), visualize.colormap('inferno')
    assert plasma.shape == inferno.shape == (256, 3) and plasma.dtype == inferno.dtype == np.uint8
    assert len({tuple(c) for c in plasma.tolist()}) == 256                      # what plasma_index relies on
    # the ends of the two maps (matplotlib's listed data: plasma floor(c * 255), inferno rint(c * 255))
    assert plasma[0].tolist() == [12, 7, 134] and plasma[255].tolist() == [239, 248, 33]
    assert inferno[0].tolist() == [0, 0, 4] and inferno[255].tolist() == [252, 255, 164]
    with open(os.path.join(ROOT, 'unimatch_amd', 'colormaps.json')) as f:
        assert set(json.load(f)) == {'matplotlib_version', 'plasma', 'inferno'}
    src = open(os.path.join(ROOT, 'unimatch_amd', 'visualize.py')).read()
    assert not re.search(r'^\s*(import|from)\s+matplotlib', src, re.M)           # the package does not need matplotlib at run time


@pytest.mark.parametrize('group', range(GROUPS))
def test_disparity_recipe_equals_the_reference_indices(group):
    g = load_golden()
    disp, want = g[f'disp_in_{group}'], g[f'disp_idx_{group}']
    for d, w in zip(disp, want):
        idx, vmin, vmax = visualize.scalar_to_index_host(d, False, visualize.MINMAX_255)
        assert idx.dtype == np.uint8 and np.array_equal(idx, w)
        assert vmin == d.min() and vmax == d.max()
    rgb, stats = visualize.disparity_to_image(torch.from_numpy(disp), return_stats=True)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == disp.shape + (3,) and tuple(stats.shape) == (len(disp), 2)
    assert np.array_equal(rgb.numpy(), visualize.colormap('inferno')[want])
    assert np.array_equal(stats.numpy(), np.stack([disp.min((1, 2)), disp.max((1, 2))], 1))
    assert torch.equal(visualize.disparity_to_image(torch.from_numpy(disp)), rgb)


@pytest.mark.parametrize('group', range(GROUPS))
def test_inverse_depth_recipe_against_the_reference_image(group):
    g = load_golden()
    depth, want_rgb = g[f'depth_in_{group}'], g[f'depth_rgb_{group}']
    rgb, stats = visualize.inverse_depth_to_image(torch.from_numpy(depth), return_stats=True)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == depth.shape + (3,)
    got, want = plasma_index(rgb.numpy()), plasma_index(want_rgb)
    for i in range(len(depth)):
        diff = np.abs(got[i] - want[i])
        share = float((diff > 0).mean())
        print(f'group {group} image {i}: max index difference {diff.max()}, share of differing pixels {share:.3g} '
              f'(numpy {g["numpy_version"]} / matplotlib {g["matplotlib_version"]})')
        assert diff.max() <= 1 and share <= 1e-3
        inv = np.float32(1.0) / depth[i]
        assert stats[i, 0].item() == inv.min() and stats[i, 1].item() == visualize.percentile95(inv)
        # the recipe's percentile against NumPy's own, whatever its version: a few ulps
        assert abs(float(stats[i, 1]) - float(np.percentile(inv, 95))) <= 8 * 2.0 ** -23 * float(stats[i, 1])


def test_percentile_definition_and_edge_cases():
    rng = np.random.default_rng(5)
    for n in (1, 2, 21, 101, 1000, 1961):
        v = rng.standard_normal(n).astype(np.float32)
        a = np.sort(v)
        k = 0.95 * (n - 1)
        lo = int(np.floor(k))
        hi = min(lo + 1, n - 1)
        want = np.float32(np.float64(a[lo]) + (np.float64(a[hi]) - np.float64(a[lo])) * (k - lo))
        assert visualize.percentile95(v) == want
        if n in (21, 101):                                                     # 0.95 (n - 1) is an integer: an element itself
            assert k == lo and want == a[lo]
    # n = 1 and a constant image: vmax == vmin, index 0 everywhere, in both modes
    for x in (np.full((1, 1), 3.5, np.float32), np.full((5, 7), -2.0, np.float32)):
        for inverse in (False, True):
            for norm in (visualize.MINMAX_255, visualize.MIN_P95_256):
                idx, vmin, vmax = visualize.scalar_to_index_host(x, inverse, norm)
                assert not idx.any() and vmin == vmax
    # min-max: the ends are 0 and 255; min-p95: everything from the percentile up is 255
    x = np.linspace(-3, 7, 200, dtype=np.float32).reshape(10, 20)
    idx, _, _ = visualize.scalar_to_index_host(x, False, visualize.MINMAX_255)
    assert idx.flat[0] == 0 and idx.flat[-1] == 255
    idx, vmin, vmax = visualize.scalar_to_index_host(x, False, visualize.MIN_P95_256)
    assert idx.flat[0] == 0 and (idx[x >= vmax] == 255).all() and (idx[x < vmax] < 255).any()
    with pytest.raises(ValueError):
        visualize.scalar_to_index_host(x, False, 'p95')
    with pytest.raises(ValueError):
        visualize.disparity_to_image(torch.zeros(4, 4))


def test_abi_declares_the_new_symbols_and_checks_arguments_without_gpu():
    header = open(os.path.join(ROOT, 'include', 'unimatch_hip.h')).read()
    for name in ('um_scalar_to_rgb', 'um_scalar_to_rgb_workspace_bytes', 'um_image_prepare_flip', 'um_pred_restore_flip'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _abi.SIGNATURES, name
    assert re.search(r'#define UM_NORM_MINMAX_255 0\b', header) and re.search(r'#define UM_NORM_MIN_P95_256 1\b', header)
    assert 'NaN' in header[header.index('Scalar map -> colour image'):header.index('#define UM_NORM_MINMAX_255')]
    lib = _abi.load()
    assert lib.um_scalar_to_rgb_workspace_bytes(0, 4, 4) == 0 and lib.um_scalar_to_rgb_workspace_bytes(1, 40000, 40000) == 0
    small, big = lib.um_scalar_to_rgb_workspace_bytes(1, 1, 1), lib.um_scalar_to_rgb_workspace_bytes(8, 1080, 1920)
    assert 0 < small < big
    fake = ctypes.c_void_p(4096)

    def call(x=fake, rgb=fake, b=1, h=4, w=4, inverse=0, norm=0, lut=fake, stats=None, ws=fake, nbytes=1 << 20):
        return lib.um_scalar_to_rgb(x, rgb, b, h, w, inverse, norm, lut, stats, ws, nbytes, None)

    assert call(x=None) == -1 and b'um_scalar_to_rgb' in lib.um_last_error_string()
    assert call(rgb=None) == -1 and call(lut=None) == -1 and call(b=0) == -1 and call(h=0) == -1 and call(norm=2) == -1
    assert call(b=70000) == -1 and call(h=40000, w=40000) == -1
    assert call(ws=None) == -3 and call(nbytes=16) == -3
    # the flip entry points refuse what the plain ones refuse
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.um_image_prepare_flip(None, 0, fake, 1, 37, 53, 0, None, None, 0, 40, 56, 1, 1, 1, None) == -1
    assert lib.um_image_prepare_flip(fake, 0, fake, 1, 37, 53, 0, f3, None, 0, 40, 56, 1, 1, 1, None) == -1
    assert lib.um_image_prepare_flip(fake, 0, fake, 1, 37, 53, 0, None, None, 0, 36, 56, 1, 1, 1, None) == -1
    assert lib.um_pred_restore_flip(fake, None, 1, 2, 40, 56, 0, 1, 1, 37, 53, 0, 0, 1, None) == -1
    assert lib.um_pred_restore_flip(fake, fake, 1, 2, 40, 56, 0, 4, 1, 37, 53, 0, 0, 1, None) == -1
    from unimatch_amd.ops import HipOps
    ops = HipOps.__new__(HipOps)
    with pytest.raises(ValueError):
        HipOps.scalar_to_rgb(ops, torch.zeros(1, 4, 4), torch.zeros(256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        HipOps.scalar_to_rgb(ops, torch.zeros(1, 4, 4), torch.zeros(256, 3, dtype=torch.uint8), norm='p95')
