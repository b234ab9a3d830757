"""GPU tests of the video mode: ``um_fwd_bwd_occlusion`` / ``um_flow_to_rgb`` against fixtures minted from the reference and an fp64
restatement, and ``UniMatch.forward_sequence`` (encoder reuse across frames) against the pairwise forward."""
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, video
from unimatch_amd.model import _warp
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_frames, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'video.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def occ_margins(fwd, bwd, alpha=0.01, beta=0.5):
    """fp64 restatement: (|fwd + bwd(p + fwd)| - thr, |bwd + fwd(p + bwd)| - thr, thr) per pixel."""
    f, b = fwd.double().cpu(), bwd.double().cpu()
    thr = alpha * (torch.norm(f, dim=1) + torch.norm(b, dim=1)) + beta
    return torch.norm(f + _warp(b, f), dim=1) - thr, torch.norm(b + _warp(f, b), dim=1) - thr, thr


def check_occ(got, want, margin, thr):
    """Every pixel where the kernel and the reference disagree lies within 1e-4 thr of the threshold (fp64)."""
    off = got.cpu() != want
    assert (margin[off].abs() <= 1e-4 * thr[off]).all(), (int(off.sum()), margin[off].abs().max().item())
    return int(off.sum())


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_occlusion_kernel_matches_reference(golden, tag):
    fwd = torch.from_numpy(golden[f'occ_fwd_in_{tag}']).to(DEV)
    bwd = torch.from_numpy(golden[f'occ_bwd_in_{tag}']).to(DEV)
    occ_f, occ_b = video.forward_backward_consistency_check(fwd, bwd)
    assert occ_f.is_cuda and occ_f.dtype == torch.float32
    mf, mb, thr = occ_margins(fwd, bwd)
    check_occ(occ_f, torch.from_numpy(golden[f'occ_fwd_{tag}']), mf, thr)
    check_occ(occ_b, torch.from_numpy(golden[f'occ_bwd_{tag}']), mb, thr)


def test_occlusion_kernel_against_fp64_odd_sizes():
    g = torch.Generator().manual_seed(5)
    for b, h, w in ((3, 33, 47), (2, 64, 97), (1, 5, 3)):
        fwd = (torch.randn(b, 2, h, w, generator=g) * 4).float()
        fwd[:, 0, :, -2:] += 40.0                                     # far out of frame on the right
        fwd[:, 1, :2] -= 30.0
        bwd = (-fwd + 0.3 * torch.randn(b, 2, h, w, generator=g)).float()
        for alpha, beta in ((0.01, 0.5), (0.05, 0.1)):
            occ_f, occ_b = video.forward_backward_consistency_check(fwd.to(DEV), bwd.to(DEV), alpha, beta)
            mf, mb, thr = occ_margins(fwd, bwd, alpha, beta)
            check_occ(occ_f, (mf > 0).float(), mf, thr)
            check_occ(occ_b, (mb > 0).float(), mb, thr)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_flow_rgb_kernel_matches_reference(golden, tag):
    flow = torch.from_numpy(golden[f'rgb_in_{tag}']).to(DEV)
    want = golden[f'rgb_{tag}']
    rgb = video.flow_to_image(flow)
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == want.shape
    got = rgb.cpu().numpy()
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert diff.max() <= 1 and (diff == 0).mean() >= 0.9999, ((diff != 0).sum(), diff.max())
    host = flow.cpu()
    unknown = ((host.abs() > 1e7).any(1)).numpy()
    assert (got[unknown] == 0).all()
    # each image by its own maximum: colouring an image alone gives the same bytes
    for i in range(flow.shape[0]):
        assert torch.equal(video.flow_to_image(flow[i:i + 1]), rgb[i:i + 1])


def test_flow_rgb_kernel_is_stateless():
    g = torch.Generator().manual_seed(9)
    a = (torch.randn(3, 2, 70, 90, generator=g) * 7).to(DEV)
    b = (torch.randn(2, 2, 130, 257, generator=g) * 30).to(DEV)       # more partial maxima per image than a
    first = video.flow_to_image(a)
    again = [video.flow_to_image(a) for _ in range(2)]
    video.flow_to_image(b)
    after = video.flow_to_image(a)
    torch.cuda.synchronize()
    assert all(torch.equal(first, r) for r in again) and torch.equal(first, after)
    want = video.flow_to_image(a.cpu())
    d = (first.cpu().short() - want.short()).abs()
    assert d.max().item() <= 1 and (d == 0).float().mean().item() >= 0.9999


# ------------------------------------------------------------------ forward_sequence
def _model(name):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    return model.to(DEV), {k: v for k, v in fk.items() if k != 'task'}


def floor_close(a, b):
    return (a - b).abs().max().item() < 1e-3 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize('name', ['gmflow_s1', 'gmflow_s2_rr6'])
def test_sequence_against_pairwise(name):
    model, kw = _model(name)
    T = 10
    frames = synth_frames(T, 128, 192, seed=77).to(DEV)
    pairwise = torch.cat([model(frames[i:i + 1], frames[i + 1:i + 2], pred_bidir_flow=True, **kw)['flow_preds'][0]
                          for i in range(T - 1)], 0).view(T - 1, 2, 2, 128, 192)
    calls = [0]
    inner = model.backbone.forward

    def counted(x, *a, **k):
        calls[0] += x.shape[0]
        return inner(x, *a, **k)
    model.backbone.forward = counted
    args = dict(pairs_per_launch=4, pred_bidir_flow=True, consistency_check=True, colorize=True, **kw)
    out = model.forward_sequence(frames, **args)
    assert calls[0] == T
    del model.backbone.forward
    assert torch.isfinite(out['flow']).all()
    for i in range(T - 1):
        assert floor_close(out['flow'][i], pairwise[i, 0]), i
        assert floor_close(out['flow_bwd'][i], pairwise[i, 1]), i
    again = model.forward_sequence(frames, **args)
    torch.cuda.synchronize()
    for key in ('flow', 'flow_bwd', 'occ_fwd', 'occ_bwd', 'flow_rgb', 'flow_bwd_rgb'):
        assert torch.equal(again[key], out[key]), key
    occ_f, occ_b = video.forward_backward_consistency_check(out['flow'], out['flow_bwd'])
    assert torch.equal(occ_f, out['occ_fwd']) and torch.equal(occ_b, out['occ_bwd'])
    assert torch.equal(video.flow_to_image(out['flow']), out['flow_rgb'])
    assert torch.equal(video.flow_to_image(out['flow_bwd']), out['flow_bwd_rgb'])
    # fed in pieces with the carry: chunks of 4 from frame 0 and frame 5 -> the same chunk shapes as one call (bitwise) ...
    a = model.forward_sequence(frames[:5], **args)
    b = model.forward_sequence(frames[5:], carry=a['carry'], **args)
    for key in ('flow', 'flow_bwd', 'occ_fwd', 'flow_rgb'):
        assert torch.equal(torch.cat([a[key], b[key]], 0), out[key]), key
    # ... other chunk shapes: within the floor
    a = model.forward_sequence(frames[:3], **args)
    b = model.forward_sequence(frames[3:], carry=a['carry'], **args)
    assert floor_close(torch.cat([a['flow'], b['flow']], 0), out['flow'])
    model.check_operand_range()


def test_sequence_parts_and_interleaving():
    """512 x 768, eight pairs per launch: the match step runs as two concurrent parts; each part is bitwise the match step of its pairs
    on the same features, and within the floor of that sub-sequence run alone; plain forwards of other geometries in between change
    nothing."""
    from unimatch_amd.streams import forward_parts
    model, kw = _model('gmflow_s1')
    T = 9
    frames = synth_frames(T, 512, 768, seed=78).to(DEV)
    assert forward_parts('flow', kw['attn_type'], 1, False, 8, 512, 768) == 2
    out = model.forward_sequence(frames, pairs_per_launch=8, **kw)['flow']
    runs = [model.forward_sequence(frames, pairs_per_launch=8, **kw)['flow'] for _ in range(2)]     # concurrent parts
    torch.cuda.synchronize()
    assert all(torch.equal(r, out) for r in runs)
    with torch.no_grad():
        feats = model._encode((frames,))
        kwm = dict(kw, pred_bidir_flow=False, task='flow', num_reg_refine=1)
        for lo, hi in ((0, 4), (4, 8)):
            stream = [torch.cat([f[lo:hi], f[lo + 1:hi + 1]], 0) for f in feats]
            part = model._match(stream, hi - lo, **kwm)['flow_preds'][0]
            assert torch.equal(part, out[lo:hi]), (lo, hi)
    model.launch_parts = 1
    try:
        for lo, hi in ((0, 4), (4, 8)):
            alone = model.forward_sequence(frames[lo:hi + 1], pairs_per_launch=8, **kw)['flow']
            assert floor_close(alone, out[lo:hi])
    finally:
        model.launch_parts = None
    small = synth_frames(3, 128, 192, seed=79).to(DEV)
    for _ in range(2):
        model(small[:2], small[1:], **kw)
        model(frames[:1, :, :256, :384].contiguous(), frames[1:2, :, :256, :384].contiguous(), **kw)
        assert torch.equal(model.forward_sequence(frames, pairs_per_launch=8, **kw)['flow'], out)
    model.check_operand_range()
