"""The transition-block entry convolution (``um_conv2d_entry_fwd``, ``conv_entry_kernel``) and the projection-shortcut normalisation
on load (``um_nhwc_instance_norm_sc``).

A stride-2 residual block of the encoder reads its input ``X = relu(instance_norm(u) + S)`` with two stride-2 convolutions only: its
3x3 ``conv1`` and its 1x1 projection shortcut, which samples the centre tap of conv1's window.  The entry kernel builds X while it
stages its operand (X is never written) and returns both convolutions; the block's output apply then normalises the raw projection
while it loads it.  Neither may change one bit:

* kernel level: ``um_nhwc_instance_norm(u, shortcut_planes)`` -> ``um_conv2d_fwd`` (3x3 / 2) + ``um_conv2d_fwd`` (1x1 / 2, bias) against
  ``um_nhwc_stats_finalize`` -> ``um_conv2d_entry_fwd``: both outputs and both statistics buffers with ``torch.equal``, both arithmetics;
* one fp64 leg that shows the new entry is right on its own;
* ``um_nhwc_instance_norm_sc`` against ``um_nhwc_instance_norm`` fed the stored normalised shortcut;
* encoder level: ``CNNEncoder`` with ``HipOps.fused_entry`` on and off, ``torch.equal``, with the launch census asserting that the
  generic kernel ran exactly one launch less per transition block ``um_conv2d_entry_supported`` admits, and a count of the
  normalisation entry points asserting the launch table (apply launches removed, finalizes unchanged); the same with fp32 shortcuts.
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


def _conv(lib, planes, wp, bias, b, h, w, cin, cout, k, stride, pad, mode):
    """um_conv2d_fwd with the epilogue's statistics -> (out, stats, parts)."""
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    parts = lib.um_conv_stats_parts(h, w, cout, k, k, stride, pad, pad)
    out = torch.empty((b * ho * wo, cout), dtype=torch.float32, device=DEV)
    st = torch.zeros(lib.um_conv_stats_bytes(b, parts, cout) // 4, dtype=torch.float32, device=DEV)
    _abi.check(lib.um_conv2d_fwd(_p(planes), _p(wp), _p(bias), _p(out), _p(st), b, h, w, cin, cout, k, k, stride, pad, pad, 0, WSHIFT, mode,
                                 _stream()), 'um_conv2d_fwd')
    return out, st, parts


def _both_paths(lib, cin, cout, hw, b, mode, geo=(3, 3, 2, 1, 1)):
    """The producing convolution (bias of several units: a halo pixel wrongly set to norm(0) instead of 0 would change the result)
    leaves u and its statistics; S, the identity shortcut, is that convolution's input.  Then the block entry through the
    normalisation pass + two convolutions, and through the entry kernel.  Returns ((t, st_t, d, st_d) of each), rc, census, inputs."""
    h, w = hw
    s = rnd(96, b, cin, h, w, scale=1.5)
    w0 = rnd(97, cin, cin, 3, 3, scale=0.06)
    w1, wpj = rnd(197, cout, cin, 3, 3, scale=0.06), rnd(297, cout, cin, 1, 1, scale=0.15)
    b0, bpj = 3.0 * rnd(98, cin), 2.0 * rnd(99, cout)
    wp0, wp1, wp2 = _weight_planes(lib, w0, mode), _weight_planes(lib, w1, mode), _weight_planes(lib, wpj, mode)
    b0d, bpd = b0.to(DEV), bpj.to(DEV)
    sp = _input_planes(lib, s, mode)
    u, stu, parts_u = _conv(lib, sp, wp0, b0d, b, h, w, cin, cin, 3, 1, 1, mode)
    # (a) the parent sequence: the apply writes X as operand planes, two convolutions read them
    xp = torch.empty(lib.um_planes_bytes(b * h * w + 1, cin, mode), dtype=torch.uint8, device=DEV)
    ws = torch.empty(max(lib.um_nhwc_norm_workspace_bytes(b, h * w, cin), 256), dtype=torch.uint8, device=DEV)
    _abi.check(lib.um_nhwc_instance_norm(_p(u), None, _p(sp), _p(xp), None, b, h * w, cin, EPS, 1, 1, _p(stu), parts_u, _p(ws), ws.numel(), mode,
                                         _stream()), 'um_nhwc_instance_norm')
    ta, sta, parts = _conv(lib, xp, wp1, None, b, h, w, cin, cout, 3, 2, 1, mode)
    da, sda, parts_d = _conv(lib, xp, wp2, bpd, b, h, w, cin, cout, 1, 2, 0, mode)
    assert parts == parts_d
    # (b) finalize + entry convolution
    ns = torch.empty((b, 2, cin), dtype=torch.float32, device=DEV)
    _abi.check(lib.um_nhwc_stats_finalize(_p(stu), parts_u, _p(ns), b, h * w, cin, EPS, _stream()), 'um_nhwc_stats_finalize')
    tb, db = (torch.full(ta.shape, float('nan'), dtype=torch.float32, device=DEV) for _ in range(2))
    stb, sdb = torch.zeros_like(sta), torch.zeros_like(sda)
    lib.um_census_enable(1)
    rc = lib.um_conv2d_entry_fwd(_p(u), _p(ns), _p(sp), _p(wp1), _p(wp2), _p(bpd), _p(tb), _p(db), _p(stb), _p(sdb), b, h, w, cin, cout, *geo,
                                 WSHIFT, mode, _stream())
    census = _abi.census(lib)
    lib.um_census_enable(0)
    torch.cuda.synchronize()
    return (ta, sta, da, sda), (tb, stb, db, sdb), rc, census, (s, w0, b0, w1, wpj, bpj)


# 64 -> 96 (NT = 3) and 96 -> 128 (NT = 4): several tiles, ragged 128-pixel tiles, odd heights / widths
CASES = [(cin, cout, hw, b) for (cin, cout) in ((64, 96), (96, 128)) for hw, b in (((64, 96), 2), ((22, 60), 3), ((31, 45), 3), ((17, 33), 2))]


@pytest.mark.parametrize('mode', [0, 1], ids=['exact', 'fast'])
@pytest.mark.parametrize('cin,cout,hw,b', CASES)
def test_entry_convolution_is_bitwise_the_parent_sequence(lib, cin, cout, hw, b, mode):
    """t, d and both tile-statistics buffers of the entry kernel equal, bit for bit, those of the two convolutions behind the
    normalisation pass (Fp16 hi | lo and Bf16 operands).  A tile width the library keeps on the parent sequence
    (um_conv2d_entry_supported == 0) must refuse the call instead: an error code and no launch."""
    h, w = hw
    pa, pb, rc, census, _ = _both_paths(lib, cin, cout, hw, b, mode)
    if not lib.um_conv2d_entry_supported(h, w, cin, cout, 3, 3, 2, 1, 1, mode):
        assert rc == -2 and census['conv_generic'] == 0, (rc, census)
        return
    assert rc == 0, lib.um_last_error_string()
    assert census['conv_generic'] == 1 and census['conv_patch'] == 0 and census['conv_patch_norm'] == 0, census
    for name, x, y in zip(('t', 't statistics', 'd', 'd statistics'), pa, pb):
        assert torch.isfinite(x).all(), name
        assert torch.equal(x, y), (name, err(x, y))


def test_entry_convolution_refuses_an_unsupported_geometry(lib):
    """Stride 1 and a 64-wide output tile: -2, an error string, and the census shows no launch."""
    for cin, cout, geo in ((64, 96, (3, 3, 1, 1, 1)), (64, 64, (3, 3, 2, 1, 1))):
        assert lib.um_conv2d_entry_supported(22, 60, cin, cout, *geo, 0) == 0
        _, (tb, _, db, _), rc, census, _ = _both_paths(lib, cin, cout, (22, 60), 2, 0, geo=geo)
        assert rc == -2 and b'um_conv2d_entry_supported' in lib.um_last_error_string()
        assert all(v == 0 for v in census.values()), census
        assert torch.isnan(tb).all() and torch.isnan(db).all()                   # nothing was written


def test_entry_convolution_matches_fp64(lib):
    """Both outputs against torch fp64 (exact arithmetic), with the tolerance form of the library's other convolution tests."""
    cin, cout, hw, b = 64, 96, (22, 60), 2
    if not lib.um_conv2d_entry_supported(*hw, cin, cout, 3, 3, 2, 1, 1, 0):
        pytest.fail('the 64 -> 96 entry is switched off: this leg has nothing to check')
    _, (tb, _, db, _), rc, _, (s, w0, b0, w1, wpj, bpj) = _both_paths(lib, cin, cout, hw, b, 0)
    assert rc == 0, lib.um_last_error_string()
    f = torch.nn.functional
    x = (f.instance_norm(f.conv2d(s.double(), w0.double(), b0.double(), padding=1), eps=EPS).relu() + s.double()).relu()
    ho, wo = (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1
    for name, got, want in (('t', tb, f.conv2d(x, w1.double(), None, stride=2, padding=1)),
                            ('d', db, f.conv2d(x, wpj.double(), bpj.double(), stride=2))):
        got = got.view(b, ho, wo, cout).permute(0, 3, 1, 2)
        e = err(got, want)[0]
        print(f'entry conv {name} vs fp64: max abs err {e:.3e}, max |want| {want.abs().max().item():.3f}')
        assert e < 4e-6 * max(1.0, want.abs().max().item()), name


@pytest.mark.parametrize('mode', [0, 1], ids=['exact', 'fast'])
@pytest.mark.parametrize('c,hw,b', [(96, (32, 48), 2), (128, (11, 23), 3)])
def test_shortcut_normalised_on_load_is_bitwise_the_stored_one(lib, c, hw, b, mode):
    """um_nhwc_instance_norm_sc (raw projection output + its tile statistics) against um_nhwc_instance_norm fed the normalised
    shortcut a pass of its own stored: planes and fp32 output with torch.equal."""
    h, w = hw
    pix = h * w
    cin = 64
    x = rnd(11, b, cin, h, w, scale=1.5)
    xp = _input_planes(lib, x, mode)
    u, stu, parts_u = _conv(lib, xp, _weight_planes(lib, rnd(12, c, cin, 3, 3, scale=0.06), mode), None, b, h, w, cin, c, 3, 1, 1, mode)
    d, std_, parts_d = _conv(lib, xp, _weight_planes(lib, rnd(13, c, cin, 1, 1, scale=0.15), mode), (2.0 * rnd(14, c)).to(DEV), b, h, w, cin, c,
                             1, 1, 0, mode)
    nbytes = lib.um_planes_bytes(b * pix + 1, c, mode)
    ws = torch.empty(max(lib.um_nhwc_norm_sc_workspace_bytes(b, pix, c), 256), dtype=torch.uint8, device=DEV)
    sc = torch.empty_like(d)
    _abi.check(lib.um_nhwc_instance_norm(_p(d), None, None, None, _p(sc), b, pix, c, EPS, 1, 0, _p(std_), parts_d, _p(ws), ws.numel(), mode,
                                         _stream()), 'um_nhwc_instance_norm')
    pa, pb = (torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(2))
    fa, fb = (torch.full(u.shape, float('nan'), dtype=torch.float32, device=DEV) for _ in range(2))
    _abi.check(lib.um_nhwc_instance_norm(_p(u), _p(sc), None, _p(pa), _p(fa), b, pix, c, EPS, 1, 1, _p(stu), parts_u, _p(ws), ws.numel(), mode,
                                         _stream()), 'um_nhwc_instance_norm')
    _abi.check(lib.um_nhwc_instance_norm_sc(_p(u), _p(d), None, _p(pb), _p(fb), b, pix, c, EPS, 1, 1, _p(stu), parts_u, _p(ws), ws.numel(), mode,
                                            _stream(), _p(std_), parts_d), 'um_nhwc_instance_norm_sc')
    torch.cuda.synchronize()
    assert torch.isfinite(fa).all() and (fa > 0).any()
    assert torch.equal(fa, fb), err(fa, fb)
    assert torch.equal(pa, pb)


def _admitted_transitions(lib, enc, h, w):
    """How many blocks of ``enc`` are stride-2 blocks with a projection whose entry the library serves at an h x w input."""
    n = 0
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1                                    # the stem
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            s = blk.conv1.stride[0]
            if blk.downsample is not None and s == 2:
                n += lib.um_conv2d_entry_supported(h, w, blk.conv1.in_channels, blk.conv1.out_channels, 3, 3, 2, 1, 1, 0)
            h, w = (h - 1) // s + 1, (w - 1) // s + 1
    return n


def _projection_blocks(enc):
    return sum(blk.downsample is not None for layer in (enc.layer1, enc.layer2, enc.layer3) for blk in layer)


class _NormLaunches:
    """Counts the normalisation launches of a forward at the C entry points: every um_nhwc_instance_norm(_sc) call launches one
    nhwc_apply_kernel; a statistics finalize is launched by um_nhwc_stats_finalize, by a normalising um_nhwc_instance_norm, and
    twice by um_nhwc_instance_norm_sc."""

    def __init__(self, monkeypatch, lib):
        self.applies = self.finalizes = 0
        norm, norm_sc, fin = lib.um_nhwc_instance_norm, lib.um_nhwc_instance_norm_sc, lib.um_nhwc_stats_finalize

        def w_norm(*a):
            self.applies += 1
            self.finalizes += int(bool(a[9]))
            return norm(*a)

        def w_norm_sc(*a):
            self.applies += 1
            self.finalizes += 2
            return norm_sc(*a)

        def w_fin(*a):
            self.finalizes += 1
            return fin(*a)

        monkeypatch.setattr(lib, 'um_nhwc_instance_norm', w_norm)
        monkeypatch.setattr(lib, 'um_nhwc_instance_norm_sc', w_norm_sc)
        monkeypatch.setattr(lib, 'um_nhwc_stats_finalize', w_fin)

    def take(self):
        out = (self.applies, self.finalizes)
        self.applies = self.finalizes = 0
        return out


def _knob_on_and_off(lib, monkeypatch, enc, ops, x, norm):
    outs, counts, launches = {}, {}, {}
    tally = _NormLaunches(monkeypatch, lib)
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(HipOps, 'fused_entry', on)
            tally.take()
            lib.um_census_enable(1)
            outs[on] = enc(x, ops, norm)
            counts[on] = _abi.census(lib)
            lib.um_census_enable(0)
            launches[on] = tally.take()
    torch.cuda.synchronize()
    return outs, counts, launches


@pytest.mark.parametrize('precision', ['exact', 'fast'])
@pytest.mark.parametrize('scales', [1, 2])
@pytest.mark.parametrize('hw', [(128, 192), (136, 264), (120, 200)])
def test_encoder_is_bitwise_the_same_with_the_knob_on_and_off(lib, monkeypatch, hw, scales, precision):
    """CNNEncoder with HipOps.fused_entry on and off: equal outputs; the generic kernel ran one launch less per transition block
    um_conv2d_entry_supported admits (two-scale models: layer3.0 is stride 1, only layer2.0 can be admitted) and as often where it
    admits none; the patch kernel's launches, on-load ones included, do not change.  The launch table: one nhwc_apply_kernel less
    per projection block (its shortcut is normalised on load) and one more less per admitted block (its input is never written);
    the statistics finalizes stay what they were."""
    torch.manual_seed(7)
    enc = CNNEncoder(128, scales).to(DEV).eval()
    ops = HipOps(precision)
    assert ops.lib is lib
    x = (rnd(5, 2, 3, *hw).abs() * 90.0).clamp(0, 255).to(DEV)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    expect = _admitted_transitions(lib, enc, *hw)
    table = [lib.um_conv2d_entry_supported(64, 96, cin, cout, 3, 3, 2, 1, 1, 0) for cin, cout in ((64, 96), (96, 128))]      # per width
    assert expect == (table[0] + table[1] if scales == 1 else table[0])
    outs, counts, launches = _knob_on_and_off(lib, monkeypatch, enc, ops, x, norm)
    assert counts[False]['conv_generic'] - counts[True]['conv_generic'] == expect, (counts, expect)
    for k in ('conv_patch', 'conv_patch_norm', 'conv_rows'):
        assert counts[True][k] == counts[False][k], (k, counts)
    # stem + six block outputs + one pass per projection shortcut (+ the format conversion in front of the two-scale trident convolution)
    if hw == (128, 192):                                     # (every conv2 normalises on load there: no middle apply)
        assert launches[False][0] == 7 + _projection_blocks(enc) + (scales > 1), launches
    assert launches[False][0] - launches[True][0] == _projection_blocks(enc) + expect, (launches, expect)
    if hw == (128, 192) and scales == 1 and expect == 2:
        assert launches[True][0] == 5                        # 9 -> 5 in the encoder: the bench forward's 11 -> 7
    assert launches[True][1] == launches[False][1], launches
    if scales == 1:
        assert launches[False][1] == 15, launches
    assert len(outs[True]) == len(outs[False]) == scales
    for a, b_ in zip(outs[True], outs[False]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b_), err(a, b_)


@pytest.mark.parametrize('scales', [1, 2])
def test_encoder_with_fp32_shortcuts_keeps_the_block_input(lib, monkeypatch, scales):
    """CNNEncoder.shortcut_f32 (the A/B knob that keeps fp32 copies for the identity shortcuts): the block in front of a stride-2
    block then holds its shortcut in fp32, not as planes, so it cannot hand its output on unnormalised -- the stride-2 block takes
    the plain convolutions (no entry launch) and only the projection's normalisation moves into the output apply.  Same bits."""
    torch.manual_seed(7)
    enc = CNNEncoder(128, scales).to(DEV).eval()
    ops = HipOps('exact')
    monkeypatch.setattr(CNNEncoder, 'shortcut_f32', True)
    x = (rnd(5, 2, 3, 128, 192).abs() * 90.0).clamp(0, 255).to(DEV)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    outs, counts, launches = _knob_on_and_off(lib, monkeypatch, enc, ops, x, norm)
    assert counts[False]['conv_generic'] == counts[True]['conv_generic'], counts
    assert launches[False][0] - launches[True][0] == _projection_blocks(enc), launches
    assert launches[True][1] == launches[False][1], launches
    for a, b_ in zip(outs[True], outs[False]):
        assert torch.equal(a, b_), err(a, b_)
