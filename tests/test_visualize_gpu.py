"""GPU tests of ``um_scalar_to_rgb`` against the host recipe of ``unimatch_amd.visualize``: colours and ``(vmin, vmax)`` must be
bit-equal, in both normalisations, with and without the inverse, on the fixtures of the reference and on inputs built to reach every
path of the radix select (ranks inside and across runs of ties, keys that differ in one digit only, negative keys, one and several
workgroups per image, per-image statistics), and nothing may depend on what the workspace held before."""
import functools

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, prepost, visualize
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_camera, synth_images, synth_state_dict
from tests.visualize_util import GROUPS, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = [(inverse, norm) for norm in (visualize.MINMAX_255, visualize.MIN_P95_256) for inverse in (False, True)]


def from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def shuffled(values, shape, seed):
    values = torch.as_tensor(values, dtype=torch.float32)
    return values[torch.randperm(values.numel(), generator=torch.Generator().manual_seed(seed))].reshape(shape).contiguous()


def ties(n, boundary, seed):
    """``n`` values on 8 levels; ranks below ``boundary`` hold levels 1..7 (equal shares), the ranks from ``boundary`` on level 8."""
    low = 1.0 + torch.arange(boundary) * 7 // boundary
    return shuffled(torch.cat([low.float(), torch.full((n - boundary,), 8.0)]) * 0.37, (1, 64, n // 64), seed)


@functools.lru_cache(maxsize=None)
def cases():
    g = torch.Generator().manual_seed(77)
    rnd = lambda *shape: torch.rand(*shape, generator=g)
    n = 64 * 64
    lo = int(np.floor(0.95 * (n - 1)))                                           # 3890; hi = 3891
    out = {f'golden_disp_{i}': torch.from_numpy(load_golden()[f'disp_in_{i}']) for i in range(GROUPS)}
    out.update({f'golden_depth_{i}': torch.from_numpy(load_golden()[f'depth_in_{i}']) for i in range(GROUPS)})
    out.update({
        '1x1x1': torch.tensor([[[2.5]]]),
        '1x1x2': torch.tensor([[[2.5, 0.75]]]),
        '1x1x21': 0.5 + 9.5 * rnd(1, 1, 21),                                     # 0.95 (n - 1) = 19: t = 0
        '1x1x101': 0.5 + 9.5 * rnd(1, 1, 101),                                   # 0.95 (n - 1) = 95
        '2x131x257': 0.5 + 9.5 * rnd(2, 131, 257),                               # three workgroups per image, odd sizes
        '1x270x480': 0.5 + 9.5 * rnd(1, 270, 480),                               # eight workgroups: the multi-block fold
        'ties_inside_one_run': ties(n, lo - 300, 1),                             # ranks lo, hi both inside the run of level 8
        'ties_across_two_runs': ties(n, lo + 1, 2),                              # rank lo ends level 7, rank hi starts level 8
        'mixed_sign': (rnd(1, 37, 53) - 0.4) * 50 + 1e-3,
        'all_negative': -0.5 - 9.5 * rnd(2, 37, 53),
        # keys equal but for the last digit (10 bits) / for the first digit (sign, exponent, two mantissa bits), both signs
        'lowest_digit_only': shuffled(from_bits(0x40490000 + np.arange(1024)), (1, 32, 32), 3),
        'highest_digit_only': shuffled(from_bits(np.concatenate([(np.arange(8, 1000, 2) << 21), 0x80000000 | (np.arange(9, 1000, 2) << 21)])),
                                       (1, 8, 124), 4),
        'ranges_apart': torch.stack([(0.5 + 9.5 * rnd(45, 67)) * s for s in (1e-2, 1.0, 1e3)], 0),
        'constant': torch.full((2, 19, 23), 3.25),
    })
    assert lo == 3890 and out['highest_digit_only'].numel() == 992
    for name, x in out.items():
        assert x.dim() == 3 and x.dtype == torch.float32 and torch.isfinite(x).all() and torch.isfinite(1 / x).all(), name
    return out


@functools.lru_cache(maxsize=None)
def host(name, inverse, norm):
    """The host recipe of a case, computed once: ``(rgb [B, H, W, 3], stats [B, 2])``."""
    cmap = 'inferno' if norm == visualize.MINMAX_255 else 'plasma'
    return visualize.scalar_to_image(cases()[name], cmap, inverse, norm, return_stats=True)


def device(x, inverse, norm):
    cmap = 'inferno' if norm == visualize.MINMAX_255 else 'plasma'
    rgb, stats = visualize.scalar_to_image(x.to(DEV), cmap, inverse, norm, return_stats=True)
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and stats.dtype == torch.float32
    return rgb.cpu(), stats.cpu()


@pytest.mark.parametrize('name', sorted(cases()))
def test_scalar_to_rgb_is_the_host_recipe_bit_for_bit(name):
    x = cases()[name]
    for inverse, norm in MODES:
        want_rgb, want_stats = host(name, inverse, norm)
        rgb, stats = device(x, inverse, norm)
        tag = f'{name} {tuple(x.shape)} inverse={inverse} {norm}'
        bits = lambda t: t.view(torch.int32)
        assert torch.equal(bits(stats), bits(want_stats)), (tag, stats, want_stats)
        assert rgb.shape == want_rgb.shape and torch.equal(rgb, want_rgb), (tag, (rgb != want_rgb).any(-1).float().mean().item())
    if name in ('1x1x1', 'constant'):                                            # vmax == vmin: index 0 in every mode
        for inverse, norm in MODES:
            rgb, stats = host(name, inverse, norm)
            table = visualize.colormap('inferno' if norm == visualize.MINMAX_255 else 'plasma')
            assert (rgb.reshape(-1, 3) == torch.from_numpy(table[0])).all() and torch.equal(stats[:, 0], stats[:, 1])


def test_selected_order_statistics_are_elements_of_the_input():
    """With t = 0 (n = 21, 101) and inside a run of ties the percentile is an input value itself; per image in a batch."""
    for name in ('1x1x21', '1x1x101', 'ties_inside_one_run', 'ranges_apart'):
        x = cases()[name]
        _, stats = device(x, False, visualize.MIN_P95_256)
        for i, image in enumerate(x):
            a = np.sort(image.numpy().ravel())
            k = 0.95 * (a.size - 1)
            lo = int(np.floor(k))
            assert a[lo] <= stats[i, 1].item() <= a[min(lo + 1, a.size - 1)] and stats[i, 0].item() == a[0]
            if k == lo or a[lo] == a[min(lo + 1, a.size - 1)]:
                assert stats[i, 1].item() == a[lo]


def test_public_functions_and_no_synchronisation():
    g = load_golden()
    disp, depth = torch.from_numpy(g['disp_in_2']).to(DEV), torch.from_numpy(g['depth_in_2']).to(DEV)
    want_d, want_z = visualize.disparity_to_image(disp.cpu()), visualize.inverse_depth_to_image(depth.cpu())
    first = visualize.disparity_to_image(disp), visualize.inverse_depth_to_image(depth, return_stats=True)      # tables, library warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got_d = visualize.disparity_to_image(disp)
        got_z, stats = visualize.inverse_depth_to_image(depth, return_stats=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(got_d.cpu(), want_d) and torch.equal(got_z.cpu(), want_z) and tuple(stats.shape) == (2, 2)
    assert torch.equal(first[0], got_d) and torch.equal(first[1][0], got_z)
    with pytest.raises(ValueError):
        visualize.disparity_to_image(disp[0])


def test_nothing_depends_on_the_workspace(monkeypatch):
    """Two calls with other launches (other sizes, the other mode) between them give equal bits, and so does a workspace that was
    filled with 0xFF before the call."""
    ops = visualize._hip()
    for name in ('2x131x257', '1x270x480', 'ties_across_two_runs'):
        x = cases()[name].to(DEV)
        for inverse, norm in MODES:
            cmap = 'inferno' if norm == visualize.MINMAX_255 else 'plasma'
            lut = visualize._device_table(cmap, x.device)
            a = ops.scalar_to_rgb(x, lut, inverse, norm, return_stats=True)
            ops.scalar_to_rgb(cases()['ranges_apart'].to(DEV), lut, not inverse, visualize.MIN_P95_256)
            ops.scalar_to_rgb(cases()['mixed_sign'].to(DEV), lut, False, visualize.MINMAX_255)
            b = ops.scalar_to_rgb(x, lut, inverse, norm, return_stats=True)
            with monkeypatch.context() as m:
                m.setattr(ops, '_ws', lambda nbytes, dev: torch.full((max(int(nbytes), 256),), 255, dtype=torch.uint8, device=dev))
                c = ops.scalar_to_rgb(x, lut, inverse, norm, return_stats=True)
            want_rgb, want_stats = host(name, inverse, norm)
            for rgb, stats in (a, b, c):
                assert torch.equal(rgb.cpu(), want_rgb) and torch.equal(stats.cpu().view(torch.int32), want_stats.view(torch.int32))


def test_inverse_depth_image_of_a_model_prediction():
    ck, fk = CONFIGS['gmdepth_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    i0, i1 = synth_images(1, 64, 96, seed=1000, kind='shift', normalized=True)
    k, pose = synth_camera(1, 64, 96)
    with torch.no_grad():
        depth = model.predict(i0.to(DEV), i1.to(DEV), intrinsics=k.to(DEV), pose=pose.to(DEV), **fk)['flow_preds'][-1]
    assert tuple(depth.shape) == (1, 64, 96) and torch.isfinite(depth).all() and (depth > 0).all()
    rgb, stats = visualize.inverse_depth_to_image(depth, return_stats=True)
    want_rgb, want_stats = visualize.inverse_depth_to_image(depth.cpu(), return_stats=True)
    assert torch.equal(rgb.cpu(), want_rgb) and torch.equal(stats.cpu().view(torch.int32), want_stats.view(torch.int32))
    assert len(torch.unique(rgb.reshape(-1, 3), dim=0)) > 8                      # an image, not a flat colour
    model.check_operand_range()
