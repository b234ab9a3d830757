"""CPU tests of the video mode: the host restatements of the two post-processing functions against fixtures minted from the
reference (tests/golden/video.npz), ``UniMatch.forward_sequence`` with the CPU oracle injected as hot-path backend (pairs, chunks
with a carry, stale carries, how many images the encoder sees), the PNG writer, and the C ABI of the two kernels without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from unimatch_amd import UniMatch, _abi, io, video
from unimatch_amd.synth import CONFIGS, synth_frames, synth_state_dict
from tests.oracle_ops import OracleOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'video.npz')
T, H, W = 6, 64, 96


def close(a, b, tol=1e-4):
    """Within ``tol * max(1, |b|max)``: the encoder batch differs, CPU convolutions re-associate with the batch size (a few fp32 ulps
    on the features) and the global-matching softmax amplifies that to ~3e-5 of the flow magnitude."""
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_occlusion_host_matches_reference(golden, tag):
    fwd, bwd = torch.from_numpy(golden[f'occ_fwd_in_{tag}']), torch.from_numpy(golden[f'occ_bwd_in_{tag}'])
    occ_f, occ_b = video.forward_backward_consistency_check(fwd, bwd)
    assert occ_f.dtype == torch.float32 and tuple(occ_f.shape) == golden[f'occ_fwd_{tag}'].shape
    assert np.array_equal(occ_f.numpy(), golden[f'occ_fwd_{tag}'])
    assert np.array_equal(occ_b.numpy(), golden[f'occ_bwd_{tag}'])
    assert 0 < golden[f'occ_fwd_{tag}'].mean() < 1                     # both outcomes present


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_flow_to_image_host_matches_reference_bitwise(golden, tag):
    flow = torch.from_numpy(golden[f'rgb_in_{tag}'])
    keep = flow.clone()
    rgb = video.flow_to_image(flow)
    assert rgb.dtype == torch.uint8
    assert np.array_equal(rgb.numpy(), golden[f'rgb_{tag}'])
    assert torch.equal(torch.nan_to_num(flow, nan=123.), torch.nan_to_num(keep, nan=123.))     # the input is not written
    # the [H, W, 2] form (the reference's own) and ndarray in -> ndarray out
    one = video.flow_to_image(golden[f'rgb_in_{tag}'][0].transpose(1, 2, 0).copy())
    assert isinstance(one, np.ndarray) and np.array_equal(one, golden[f'rgb_{tag}'][0])


def test_flow_to_image_golden_covers_the_branches(golden):
    flow = golden['rgb_in_a']
    assert (np.abs(flow) > 1e7).any() and np.isnan(flow).any() and not flow[1].any()
    assert str(golden['numpy_version'])
    # the NaN image's divisor is -1 + eps: its radii straddle 1
    rad = np.sqrt(flow[4, 0].astype(np.float64) ** 2 + flow[4, 1].astype(np.float64) ** 2)
    assert (rad > 1).sum() > 100 and (rad[1:] <= 1).sum() > 100
    # unknown flow is black
    assert (golden['rgb_a'][0, 5, 7] == 0).all() and (golden['rgb_a'][0, 30, 40] == 0).all()


def test_colour_wheel():
    wheel = video.colour_wheel()
    assert wheel.shape == (55, 3)
    assert tuple(wheel[0]) == (255, 0, 0) and tuple(wheel[15]) == (255, 255, 0) and tuple(wheel[21]) == (0, 255, 0)
    assert tuple(wheel[36]) == (0, 0, 255) and tuple(wheel[49]) == (255, 0, 255) and tuple(wheel[54]) == (255, 0, 43)


def test_write_png8_roundtrip(tmp_path):
    pil = pytest.importorskip('PIL.Image')
    rgb = np.random.default_rng(0).integers(0, 256, (7, 11, 3), dtype=np.uint8)
    grey = rgb[..., 0].copy()
    io.write_png8(tmp_path / 'rgb.png', rgb)
    io.write_png8(tmp_path / 'grey.png', grey)
    assert np.array_equal(np.array(pil.open(tmp_path / 'rgb.png')), rgb)
    assert np.array_equal(np.array(pil.open(tmp_path / 'grey.png')), grey)


# ------------------------------------------------------------------ forward_sequence with the oracle backend
def _model(name='gmflow_s1'):
    ck, fk = CONFIGS[name]
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02))
    model.bind_ops(OracleOps())
    kw = {k: v for k, v in fk.items() if k != 'task'}
    return model, kw


class EncoderCount:
    """Wraps the backbone's forward and sums the batch sizes it sees."""

    def __init__(self, model):
        self.images = 0
        inner = model.backbone.forward

        def counted(x, *a, **k):
            self.images += x.shape[0]
            return inner(x, *a, **k)
        model.backbone.forward = counted


@pytest.fixture(scope='module')
def seq():
    model, kw = _model()
    frames = synth_frames(T, H, W, seed=2000)
    pairwise = torch.cat([model(frames[i:i + 1], frames[i + 1:i + 2], **kw)['flow_preds'][0] for i in range(T - 1)], 0)
    return model, kw, frames, pairwise


def test_sequence_matches_pairwise(seq):
    model, kw, frames, pairwise = seq
    for step in (8, 2, 1):
        out = model.forward_sequence(frames, pairs_per_launch=step, **kw)
        assert tuple(out['flow'].shape) == (T - 1, 2, H, W)
        assert set(out) == {'flow', 'carry'}
        assert close(out['flow'], pairwise), step


def test_encoder_sees_each_frame_once(seq):
    model, kw, frames, _ = seq
    count = EncoderCount(model)
    model.forward_sequence(frames, pairs_per_launch=2, **kw)
    assert count.images == T
    count.images = 0
    for i in range(T - 1):                                            # the reference's protocol: every interior frame twice
        model(frames[i:i + 1], frames[i + 1:i + 2], **kw)
    assert count.images == 2 * (T - 1)
    del model.backbone.forward


def test_chunks_with_carry_equal_one_call(seq):
    model, kw, frames, _ = seq
    whole = model.forward_sequence(frames, pairs_per_launch=8, pred_bidir_flow=True, consistency_check=True, colorize=True, **kw)
    count = EncoderCount(model)
    a = model.forward_sequence(frames[:4], pairs_per_launch=8, pred_bidir_flow=True, consistency_check=True, colorize=True, **kw)
    b = model.forward_sequence(frames[4:], pairs_per_launch=8, pred_bidir_flow=True, consistency_check=True, colorize=True,
                               carry=a['carry'], **kw)
    del model.backbone.forward
    assert count.images == T                                          # the carried frame is not encoded again
    assert b['flow'].shape[0] == 2 and a['flow'].shape[0] == 3
    for key in ('flow', 'flow_bwd', 'occ_fwd', 'occ_bwd', 'flow_rgb', 'flow_bwd_rgb'):
        joined = torch.cat([a[key], b[key]], 0)
        if joined.dtype == torch.uint8:
            assert torch.equal(joined, whole[key]), key
        else:
            assert close(joined, whole[key]), key


def test_bidirectional_keys_and_post_processing(seq):
    model, kw, frames, pairwise = seq
    out = model.forward_sequence(frames, pairs_per_launch=3, pred_bidir_flow=True, consistency_check=True, colorize=True, **kw)
    assert set(out) == {'flow', 'flow_bwd', 'occ_fwd', 'occ_bwd', 'flow_rgb', 'flow_bwd_rgb', 'carry'}
    assert tuple(out['flow_bwd'].shape) == (T - 1, 2, H, W) and tuple(out['occ_fwd'].shape) == (T - 1, H, W)
    assert tuple(out['flow_rgb'].shape) == (T - 1, H, W, 3) and out['flow_rgb'].dtype == torch.uint8
    ref = model(frames[1:2], frames[2:3], pred_bidir_flow=True, **kw)['flow_preds'][0]       # [forward; backward] of pair 1
    assert close(out['flow'][1], ref[0]) and close(out['flow_bwd'][1], ref[1])
    occ_f, occ_b = video.forward_backward_consistency_check(out['flow'], out['flow_bwd'])
    assert torch.equal(occ_f, out['occ_fwd']) and torch.equal(occ_b, out['occ_bwd'])
    assert torch.equal(video.flow_to_image(out['flow']), out['flow_rgb'])
    assert torch.equal(video.flow_to_image(out['flow_bwd']), out['flow_bwd_rgb'])
    with pytest.raises(AssertionError):
        model.forward_sequence(frames, consistency_check=True, **kw)


def test_stale_carry_is_encoded_again():
    model, kw = _model()
    frames = synth_frames(T, H, W, seed=2001)
    a = model.forward_sequence(frames[:3], **kw)
    with torch.no_grad():
        model.transformer.layers[0].self_attn.q_proj.weight.mul_(1.5)           # in-place edit: the carry's features are stale
    count = EncoderCount(model)
    b = model.forward_sequence(frames[3:], carry=a['carry'], **kw)
    del model.backbone.forward
    assert count.images == T - 3 + 1                                  # the carried frame went through the encoder again
    fresh = model.forward_sequence(frames[2:], **kw)
    assert torch.equal(b['flow'], fresh['flow'])
    # an edit that only the encoder sees is caught too
    c = model.forward_sequence(frames[:3], **kw)
    with torch.no_grad():
        model.backbone.conv1.weight.mul_(0.5)
    d = model.forward_sequence(frames[3:], carry=c['carry'], **kw)
    assert torch.equal(d['flow'], model.forward_sequence(frames[2:], **kw)['flow'])
    # another model's carry is never trusted, a carry of another geometry is refused
    other, _ = _model()
    count = EncoderCount(other)
    other.forward_sequence(frames[3:], carry=c['carry'], **kw)
    assert count.images == T - 3 + 1
    with pytest.raises(ValueError):
        model.forward_sequence(synth_frames(2, 32, 64), carry=c['carry'], **kw)


def test_two_scale_refinement_sequence():
    """Per-scale features and the refinement's pre-Transformer tokens come from per-frame features.  Two scales + refinement with
    synthetic weights is ill-conditioned (a batch of two pairs differs from the pairs alone by up to 0.7 px here), so the pairs are
    compared with the pairwise call of the same chunk, by the mean error test_host_logic_cpu allows for this configuration."""
    model, kw = _model('gmflow_s2_rr6')
    kw['num_reg_refine'] = 2
    frames = synth_frames(4, 128, 192, seed=2002)
    out = model.forward_sequence(frames, pairs_per_launch=2, pred_bidir_flow=True, **kw)
    for lo, hi in ((0, 2), (2, 3)):
        ref = model(frames[lo:hi], frames[lo + 1:hi + 1], pred_bidir_flow=True, **kw)['flow_preds'][0]
        n = hi - lo
        assert (out['flow'][lo:hi] - ref[:n]).abs().mean().item() < 2e-2
        assert (out['flow_bwd'][lo:hi] - ref[n:]).abs().mean().item() < 2e-2
    last = model(frames[2:3], frames[3:4], pred_bidir_flow=True, **kw)['flow_preds'][0]
    assert torch.equal(out['flow'][2:], last[:1]) and torch.equal(out['flow_bwd'][2:], last[1:])   # same launches: bitwise


def test_sequence_argument_errors(seq):
    model, kw, frames, _ = seq
    with pytest.raises(ValueError):
        model.forward_sequence(frames[:1], **kw)
    with pytest.raises(ValueError):
        model.forward_sequence(frames[:, :2], **kw)
    with pytest.raises(ValueError):
        model.forward_sequence(frames, pairs_per_launch=0, **kw)


# ------------------------------------------------------------------ C ABI without a GPU
def test_video_symbols_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'unimatch_hip.h')).read()
    for name in ('um_fwd_bwd_occlusion', 'um_flow_to_rgb', 'um_flow_to_rgb_workspace_bytes'):
        assert f'{name}(' in text and hasattr(lib, name) and name in _abi.SIGNATURES


def test_video_abi_argument_errors_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(16)
    assert lib.um_flow_to_rgb_workspace_bytes(2, 96, 128) == 2 * 3 * 4          # ceil(12288 / 4096) partial maxima per image
    assert lib.um_flow_to_rgb_workspace_bytes(0, 96, 128) == 0
    assert lib.um_fwd_bwd_occlusion(None, p, p, p, 1, 8, 8, 0.01, 0.5, None) == -1
    assert lib.um_fwd_bwd_occlusion(p, p, p, p, 1, 1, 8, 0.01, 0.5, None) == -1     # grid_sample align_corners needs H, W >= 2
    assert lib.um_fwd_bwd_occlusion(p, p, p, p, 0, 8, 8, 0.01, 0.5, None) == -1
    assert lib.um_flow_to_rgb(p, p, 0, 8, 8, p, 1024, None) == -1
    assert lib.um_flow_to_rgb(None, p, 1, 8, 8, p, 1024, None) == -1
    assert lib.um_flow_to_rgb(p, p, 1, 8, 8, p, 0, None) == -3                   # workspace too small
    assert lib.um_flow_to_rgb(p, p, 1, 8, 8, None, 1024, None) == -3
    assert b'workspace' in lib.um_last_error_string()
