"""The normalise-on-load operand path of the 3x3 patch convolution (``um_conv2d_norm_fwd``, ``conv_patch_norm_kernel``).

A residual block of the encoder runs ``conv1 -> InstanceNorm + ReLU -> conv2``; the on-load path lets ``conv2`` read conv1's fp32
output and normalise while it stages its operand, so the normalisation's pass over memory disappears.  It must not change one bit:

* kernel level: ``conv1 (stats) -> um_nhwc_instance_norm(planes) -> um_conv2d_fwd`` against ``conv1 (stats) -> um_nhwc_stats_finalize
  -> um_conv2d_norm_fwd``, output and emitted tile statistics compared with ``torch.equal`` in both arithmetics;
* one fp64 leg that shows the new entry is right on its own;
* encoder level: ``CNNEncoder`` with ``HipOps.norm_on_load`` on and off, ``torch.equal``, with the launch census asserting that
  the on-load kernel ran exactly as often as ``um_conv2d_norm_supported`` said it would.
"""
import pytest
import torch

from unimatch_amd import _abi
from unimatch_amd.encoder import CNNEncoder
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WSHIFT = 10
EPS = 1e-5


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def err(a, b):
    d = (a.double().cpu() - b.double().cpu()).abs()
    return d.max().item(), d.mean().item()


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def lib():
    HipOps('exact')                      # loads the library, fails loudly without a GPU
    return _abi.load()


def _weight_planes(lib, wt, mode):
    cout, cin, kh, kw = wt.shape
    w2 = wt.to(DEV).float().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous()
    planes = torch.empty(lib.um_planes_bytes(cout, kh * kw * cin, mode), dtype=torch.uint8, device=DEV)
    _abi.check(lib.um_weight_planes(_p(w2), _p(planes), cout, kh * kw * cin, WSHIFT, mode, _stream()), 'um_weight_planes')
    return planes


def _input_planes(lib, x, mode):
    b, c, h, w = x.shape
    xd = x.to(DEV).contiguous()
    planes = torch.empty(lib.um_planes_bytes(b * h * w + 1, c, mode), dtype=torch.uint8, device=DEV)
    _abi.check(lib.um_nchw_to_nhwc(_p(xd), _p(planes), None, b, c, h * w, mode, _stream()), 'um_nchw_to_nhwc')
    return planes


def _conv(lib, planes, wp, bias, b, h, w, cin, cout, mode):
    """um_conv2d_fwd, 3x3 / stride 1 / pad 1, with the epilogue's statistics -> (out, stats, parts)."""
    parts = lib.um_conv_stats_parts(h, w, cout, 3, 3, 1, 1, 1)
    out = torch.empty((b * h * w, cout), dtype=torch.float32, device=DEV)
    st = torch.zeros(lib.um_conv_stats_bytes(b, parts, cout) // 4, dtype=torch.float32, device=DEV)
    _abi.check(lib.um_conv2d_fwd(_p(planes), _p(wp), _p(bias), _p(out), _p(st), b, h, w, cin, cout, 3, 3, 1, 1, 1, 0, WSHIFT, mode,
                                 _stream()), 'um_conv2d_fwd')
    return out, st, parts


def _both_paths(lib, c, hw, b, mode, cin=64):
    """conv1 (bias of several units: a halo pixel wrongly set to norm(0) instead of 0 would change the result), then conv2 through
    the normalisation pass and through the on-load kernel.  Returns the two (output, statistics) pairs and the inputs."""
    h, w = hw
    x = rnd(96, b, cin, h, w, scale=1.5)
    w1, w2 = rnd(97, c, cin, 3, 3, scale=0.06), rnd(197, c, c, 3, 3, scale=0.06)
    bs = 3.0 * rnd(98, c)
    wp1, wp2 = _weight_planes(lib, w1, mode), _weight_planes(lib, w2, mode)
    bsd = bs.to(DEV)
    t, st1, parts = _conv(lib, _input_planes(lib, x, mode), wp1, bsd, b, h, w, cin, c, mode)
    # (a) the normalisation pass writes operand planes, the convolution reads them
    tp = torch.empty(lib.um_planes_bytes(b * h * w + 1, c, mode), dtype=torch.uint8, device=DEV)
    ws = torch.empty(max(lib.um_nhwc_norm_workspace_bytes(b, h * w, c), 256), dtype=torch.uint8, device=DEV)
    _abi.check(lib.um_nhwc_instance_norm(_p(t), None, None, _p(tp), None, b, h * w, c, EPS, 1, 1, _p(st1), parts, _p(ws), ws.numel(), mode,
                                         _stream()), 'um_nhwc_instance_norm')
    ua, sta, _ = _conv(lib, tp, wp2, None, b, h, w, c, c, mode)
    # (b) finalize + on-load convolution
    ns = torch.empty((b, 2, c), dtype=torch.float32, device=DEV)
    _abi.check(lib.um_nhwc_stats_finalize(_p(st1), parts, _p(ns), b, h * w, c, EPS, _stream()), 'um_nhwc_stats_finalize')
    ub = torch.full((b * h * w, c), float('nan'), dtype=torch.float32, device=DEV)
    stb = torch.zeros_like(sta)
    lib.um_census_enable(1)
    rc = lib.um_conv2d_norm_fwd(_p(t), _p(ns), 1, _p(wp2), None, _p(ub), _p(stb), b, h, w, c, c, 3, 3, 1, 1, 1, 0, WSHIFT, mode, _stream())
    census = _abi.census(lib)
    lib.um_census_enable(0)
    torch.cuda.synchronize()
    return (ua, sta), (ub, stb), rc, census, (x, w1, w2, bs)


CASES = [(64, (16, 64), 3), (96, (16, 64), 3), (128, (24, 32), 3),
         (64, (22, 60), 3), (96, (30, 31), 3), (128, (15, 90), 3),           # ragged tiles: halo pixels and whole waves outside the image
         (64, (64, 96), 3), (96, (64, 96), 3), (128, (64, 96), 3)]           # several tiles in both directions, per tile width


@pytest.mark.parametrize('mode', [0, 1], ids=['exact', 'fast'])
@pytest.mark.parametrize('c,hw,b', CASES)
def test_on_load_convolution_is_bitwise_the_normalised_one(lib, c, hw, b, mode):
    """Output and tile statistics of the on-load convolution equal, bit for bit, those of the convolution behind the
    normalisation pass (Fp16 hi | lo and Bf16 operands).  A tile width the library keeps on the normalisation pass
    (um_conv2d_norm_supported == 0) must refuse the call instead: an error code and no launch."""
    h, w = hw
    assert lib.um_conv_stats_parts(h, w, c, 3, 3, 1, 1, 1) == 2 * ((h + 7) // 8) * ((w + 31) // 32)      # a patch-kernel geometry
    (ua, sta), (ub, stb), rc, census, _ = _both_paths(lib, c, hw, b, mode)
    if not lib.um_conv2d_norm_supported(h, w, c, c, 3, 3, 1, 1, 1, mode):
        assert rc == -2 and census['conv_patch_norm'] == 0 and census['conv_patch'] == 0, (rc, census)
        return
    assert rc == 0, lib.um_last_error_string()
    assert census['conv_patch_norm'] == 1 and census['conv_patch'] == 1, census
    assert torch.isfinite(ua).all()
    assert torch.equal(ua, ub), err(ua, ub)
    assert torch.equal(sta, stb), err(sta, stb)


def test_on_load_convolution_matches_fp64(lib):
    """conv2d(relu(instance_norm(conv2d(x)))) in torch fp64 against conv1 -> finalize -> on-load conv2 (exact arithmetic), with the
    tolerance form of the library's other convolution tests."""
    c, hw, b = 64, (22, 60), 2
    _, (ub, _), rc, _, (x, w1, w2, bs) = _both_paths(lib, c, hw, b, 0)
    assert rc == 0, lib.um_last_error_string()
    f = torch.nn.functional
    want = f.conv2d(f.instance_norm(f.conv2d(x.double(), w1.double(), bs.double(), padding=1), eps=EPS).relu(), w2.double(), None,
                    padding=1)
    got = ub.view(b, hw[0], hw[1], c).permute(0, 3, 1, 2)
    e = err(got, want)[0]
    print(f'on-load conv vs fp64: max abs err {e:.3e}, max |want| {want.abs().max().item():.3f}')
    assert e < 4e-6 * max(1.0, want.abs().max().item())


def _supported_blocks(lib, enc, h, w):
    """How many residual blocks of ``enc`` have a conv2 the on-load kernel serves at an h x w input (stem: stride 2)."""
    n = 0
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            s = blk.conv1.stride[0]
            h, w = (h - 1) // s + 1, (w - 1) // s + 1
            c = blk.conv1.out_channels
            n += lib.um_conv2d_norm_supported(h, w, c, c, 3, 3, 1, 1, 1, 0)
    return n


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('scales', [1, 2])
@pytest.mark.parametrize('hw', [(128, 192), (136, 264), (120, 200)])
def test_encoder_is_bitwise_the_same_with_the_knob_on_and_off(lib, monkeypatch, hw, scales, precision):
    """CNNEncoder with HipOps.norm_on_load on and off: equal outputs, and the on-load kernel ran exactly where
    um_conv2d_norm_supported said yes: every block at 128 x 192, some blocks at 136 x 264 (conv_pick's 3/4-coverage rule admits
    the 68 x 132 map only), none at 120 x 200."""
    torch.manual_seed(7)
    enc = CNNEncoder(128, scales).to(DEV).eval()
    ops = HipOps(precision)
    x = (rnd(5, 2, 3, *hw).abs() * 90.0).clamp(0, 255).to(DEV)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    expect = _supported_blocks(lib, enc, *hw)
    table = [lib.um_conv2d_norm_supported(64, 96, c, c, 3, 3, 1, 1, 1, 0) for c in (64, 96, 128)]     # the per-width decision
    if hw == (128, 192):
        assert expect == 2 * sum(table)                      # 6 per call with all three tile widths enabled
    elif hw == (136, 264):
        assert expect == 2 * table[0]
    else:
        assert expect == 0
    outs, counts = {}, {}
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(HipOps, 'norm_on_load', on)
            lib.um_census_enable(1)
            outs[on] = enc(x, ops, norm)
            counts[on] = _abi.census(lib)
            lib.um_census_enable(0)
    torch.cuda.synchronize()
    assert counts[False]['conv_patch_norm'] == 0 and counts[True]['conv_patch_norm'] == expect, (counts, expect)
    assert counts[True]['conv_patch'] == counts[False]['conv_patch']                # the same tiling either way
    assert len(outs[True]) == len(outs[False]) == scales
    for a, b_ in zip(outs[True], outs[False]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b_), err(a, b_)
