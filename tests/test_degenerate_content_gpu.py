"""Degenerate content (tests/degenerate_content.py) on the GPU: flat, black, letterboxed, noise-only and repeated frames against fp64.

Every other input of the suite is textured noise.  This file drives the kernels into the corners that video content reaches:

* statistics with no spread -- the InstanceNorm kernels (``ops.nhwc_norm``, ``ops.instance_norm``), the statistics epilogue of the
  convolution, the norm-on-load and entry convolutions, the stem, and the LayerNorm epilogues of ``linear_ln``, ``ffn_ln`` and
  ``window_attention_merge`` -- on the eight channel patterns ``P0 .. P7`` of ``channel_patterns`` and on zero / identical / offset rows;
* softmaxes with nothing to choose from -- identical, all-zero, two-level and duplicated tokens give exactly equal logits in the global
  and local matching, the propagation, the window attention and the matching statistics (``best``: the lowest index on a tie);
* whole forwards and ``forward_sequence`` on the image kinds of ``KINDS``, under the gates of tests/test_forward_flags_gpu.py.

Gates.  Each test takes the tolerance of the existing test of the same entry point (named in its docstring).
P0, P1, P2, P5, P6, P7: that tolerance times ``max(1, |want|max)`` over the pattern's channels (P1's outlier has a z-score near
``sqrt(N)``).  P3, P4 (mean / sigma = 10^2, 10^3): the input's conditioning sets the accuracy, so the gate is
``2 x max|fp32 torch - fp64| + the existing tolerance``, the fp32 figure measured here from the reference expression on the same tensor
(the 2 x is the margin of test_exact_mode_operand_scale_sweep).  P0 with no ReLU and no shortcut: fp64 says exactly 0, the kernel may
round the mean once, ``|y| <= 2 |c| 2^-23 / sqrt(eps)``.  Lines that start with ``DC|`` are the figures of profiles/degenerate_content.txt.
"""
import math

import pytest
import torch

from oracle import hotpath as hp
from tests import degenerate_content as dc
from tests import forward_flags as ff
from tests.dispatch_boundaries import ffn_reference, merged_layer_reference
from tests.test_forward_flags_gpu import check_gates, run_gpu
from unimatch_amd import UniMatch, _abi, confidence
from unimatch_amd.ops import HipOps
from unimatch_amd.synth import CONDITIONED, CONFIGS, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 128
EPS = 1e-5
F = torch.nn.functional
ILL = (3, 4)                                   # patterns whose conditioning sets the accuracy; the others: the entry point's tolerance


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tok(fmap):
    return fmap.flatten(2).transpose(1, 2).contiguous()


def err(a, b):
    d = (a.double().cpu() - b.double().cpu()).abs()
    return d.max().item(), d.mean().item()


def record(*fields):
    print('\nDC|' + '|'.join(f'{f:.3e}' if isinstance(f, float) else str(f) for f in fields))


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


@pytest.fixture(scope='module')
def lib(ops):
    return ops.lib


def census(lib, fn):
    lib.um_census_enable(1)
    try:
        out = fn()
    finally:
        counts = _abi.census(lib)
        lib.um_census_enable(0)
    return out, counts


def nchw(t, b, h, w):
    return t.view(b, h, w, -1).permute(0, 3, 1, 2)


# ================================================================== statistics kernels
def pattern_gates(what, got, want64, want32, tol, also=None, carry=None):
    """``got``, ``want64``, ``want32`` NCHW (the kernel, the fp64 reference, the same expression in fp32 torch): the module's gates per
    pattern.  ``also``: the fp64 value of a second, well-conditioned normalisation that is added to the first in ``want64`` -- the
    error of a sum is at most the sum of the errors, so its gate (``tol`` times its ``max(1, |.|max)``) is added to the bound.
    ``carry``: only the first ``carry`` channels hold a pattern; the others (zero-mean mixtures) are gated as one textured group, 'mix'.
    Returns {pattern: (error, bound)}."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    pat = dc.pattern_of(got.shape[1])
    if carry is not None:
        pat[carry:] = dc.PATTERNS
    out = {}
    for p in range(dc.PATTERNS + 1):
        sel = pat == p
        if not bool(sel.any()):
            continue
        e = (got[:, sel] - want64[:, sel]).abs().max().item()
        if p in ILL:
            e32 = (want32[:, sel].double() - want64[:, sel]).abs().max().item()
            bound, ref = 2 * e32 + tol, e32
        else:
            bound = ref = tol * max(1.0, want64[:, sel].abs().max().item())
        if also is not None:
            bound += tol * max(1.0, also[:, sel].abs().max().item())
        record(what, f'P{p}' if p < dc.PATTERNS else 'mix', e, ref, bound)
        out[p] = (e, bound)
    bad = {p: v for p, v in out.items() if not v[0] <= v[1]}
    assert not bad, (what, bad)
    return out


def constant_channel_gate(what, got, x, carry=None, slack=0.0):
    """P0 channels of a normalisation of ``x`` (NCHW on the host: what the kernel normalised) with no shortcut: every such plane of
    ``x`` is exactly one value ``c`` (asserted), so ``|y| <= 2 |c| 2^-23 / sqrt(eps)`` (+ ``slack``, for
    a caller whose ``got`` went through one more fp32 addition); records whether they are 0."""
    got = got.double().cpu()
    carry = got.shape[1] if carry is None else carry
    exact = True
    for ch in torch.nonzero(dc.pattern_of(carry) == 0).flatten().tolist():
        for n in range(got.shape[0]):
            c = x[n, ch, 0, 0].item()
            assert bool((x[n, ch] == c).all()), (what, n, ch)
            worst = got[n, ch].abs().max().item()
            bound = 2 * abs(c) * 2.0 ** -23 / math.sqrt(EPS) + slack
            exact = exact and worst == 0.0
            assert worst <= bound, (what, n, ch, c, worst, bound)
    record(what, 'P0 exactly zero', exact)


NORM_SHAPES = [(2, 64, 37, 29), (3, 128, 5, 7), (1, 8, 520, 512)]


@pytest.mark.parametrize('shape', NORM_SHAPES)
def test_nhwc_norm_on_the_patterns(ops, shape):
    """``ops.nhwc_norm`` with its own statistics pass (test_nhwc_instance_norm: 2e-5; planes 2e-6 relative, padding row zero): with and
    without ReLU, with ``shortcut`` and with ``shortcut_planes``, both output forms.  (1, 8, 520, 512) has more than 1024 statistics
    parts per image: the two-pass merge."""
    b, c, h, w = shape
    x = dc.channel_patterns(b, c, h, w, seed=4100)
    sc = rnd(4101, b, c, h, w)
    _, xf = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=False, want_f32=True)
    assert torch.equal(nchw(xf, b, h, w).cpu(), x)
    _, scf = ops.nchw_to_nhwc(sc.to(DEV).contiguous(), want_planes=False, want_f32=True)
    n64, n32 = F.instance_norm(x.double(), eps=EPS), F.instance_norm(x, eps=EPS)
    rows = b * h * w
    for relu, shortcut in ((True, None), (False, None), (True, scf)):
        want64, want32 = (n64.relu(), n32.relu()) if relu else (n64, n32)
        if shortcut is not None:
            want64, want32 = (want64 + sc.double()).relu(), (want32 + sc).relu()
        planes, f32 = ops.nhwc_norm(xf, b, h * w, relu=relu, shortcut=shortcut, want_planes=True, want_f32=True)
        what = f'nhwc_norm {shape} relu={int(relu)} shortcut={int(shortcut is not None)}'
        pattern_gates(what, nchw(f32, b, h, w), want64, want32, 2e-5)
        if not relu:
            constant_channel_gate(what, nchw(f32, b, h, w), x)
        pl = planes.view(torch.float16).view(2, rows + 1, c).float()
        assert torch.isfinite(pl).all()
        assert torch.equal(pl[:, rows], torch.zeros(2, c, device=DEV))              # the padding row
        assert (pl[:, :rows].sum(0) - f32).abs().max().item() < 2e-6 * max(1.0, f32.abs().max().item())
    scp, _ = ops.nhwc_norm(scf, b, h * w, normalize=False, relu=False, want_planes=True)
    _, f32 = ops.nhwc_norm(xf, b, h * w, relu=True, shortcut_planes=scp, want_planes=False, want_f32=True)
    pattern_gates(f'nhwc_norm {shape} shortcut_planes', nchw(f32, b, h, w), (n64.relu() + sc.double()).relu(), (n32.relu() + sc).relu(), 2e-5)


# the NCHW kernel takes planes of a multiple of 4 pixels only (every encoder map qualifies; it refuses others): the two small shapes are
# the nearest such ones -- an odd width kept (1044 pixels: 261 float4, a ragged last register slot) and 28 pixels (less than a wave)
NCHW_SHAPES = [(2, 64, 36, 29), (3, 128, 4, 7), (1, 8, 520, 512)]


def test_nchw_instance_norm_refuses_other_plane_sizes(ops):
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.instance_norm(torch.zeros(2, 64, 37, 29, device=DEV))


@pytest.mark.parametrize('shape', NCHW_SHAPES)
def test_nchw_instance_norm_on_the_patterns(ops, shape):
    """``ops.instance_norm``, the NCHW kernel (test_fused_instance_norm: 2e-6): plain, ReLU, shortcut.  (1, 8, 520, 512) takes the
    streaming variant, the other two the register-resident one."""
    b, c, h, w = shape
    x = dc.channel_patterns(b, c, h, w, seed=4200)
    sc = rnd(4201, b, c, h, w)
    n64, n32 = F.instance_norm(x.double(), eps=EPS), F.instance_norm(x, eps=EPS)
    xd = x.to(DEV)
    got = ops.instance_norm(xd, relu=False)
    pattern_gates(f'instance_norm {shape} plain', got, n64, n32, 2e-6)
    constant_channel_gate(f'instance_norm {shape} plain', got, x)
    pattern_gates(f'instance_norm {shape} relu', ops.instance_norm(xd, relu=True), n64.relu(), n32.relu(), 2e-6)
    pattern_gates(f'instance_norm {shape} shortcut', ops.instance_norm(xd, relu=True, shortcut=sc.to(DEV)), (n64.relu() + sc.double()).relu(),
                  (n32.relu() + sc).relu(), 2e-6)


def norm_of_own_output(y, b, ho, wo):
    """fp64 and fp32 torch InstanceNorm of a kernel's own fp32 NHWC output read back: the statistics alone are under test, not the
    operand rounding of the GEMM in front of them (which ``rstd`` legitimately amplifies)."""
    ym = nchw(y, b, ho, wo).cpu().contiguous()
    return F.instance_norm(ym.double(), eps=EPS), F.instance_norm(ym, eps=EPS)


@pytest.mark.parametrize('cout,hw,stride', [(64, (15, 21), 1), (96, (7, 9), 1), (64, (22, 60), 1), (64, (47, 63), 2)])
def test_conv_epilogue_statistics_on_the_patterns(ops, cout, hw, stride):
    """``ops.conv2d_nhwc(stats=True)`` -> ``ops.nhwc_norm(conv_stats=)`` (test_conv_epilogue_statistics_feed_the_norm: 3e-5 against
    fp64, 1e-5 against the norm's own pass), the patterns in the convolution's OUTPUT (asserted on the output read back: constant P0
    planes, P6 variance far below eps, P3 / P4 at mean / sigma above 50 / 500) and the constant-channel gate on both statistics routes.
    At 96 outputs the channels beyond the 64 inputs carry no pattern: group 'mix'."""
    b, cin, (h, w) = 3, 64, hw
    x = dc.channel_patterns(b, cin, h, w, seed=4300)
    wt, bs = dc.pattern_conv_weights(cout, cin, 3, 4301)
    planes, _ = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=True)
    y, ho, wo = ops.conv2d_nhwc((planes, b, h, w, cin), wt.to(DEV), bs.to(DEV), stride, (1, 1), stats=True)
    assert ops.last_conv_stats is not None
    _, got = ops.nhwc_norm(y, b, ho * wo, relu=False, want_planes=False, want_f32=True, conv_stats=ops.last_conv_stats)
    _, own = ops.nhwc_norm(y, b, ho * wo, relu=False, want_planes=False, want_f32=True)
    n64, n32 = norm_of_own_output(y, b, ho, wo)
    ym = nchw(y, b, ho, wo).cpu()
    dc.check_output_patterns(ym, cin)
    what = f'conv epilogue {cout} {hw} /{stride}'
    pattern_gates(what, nchw(got, b, ho, wo), n64, n32, 3e-5, carry=cin)
    constant_channel_gate(what, nchw(got, b, ho, wo), ym, carry=cin)
    pattern_gates(what + ' own pass', nchw(own, b, ho, wo), n64, n32, 3e-5, carry=cin)
    constant_channel_gate(what + ' own pass', nchw(own, b, ho, wo), ym, carry=cin)
    # the two statistics routes against each other: the existing 1e-5 with the same scaling, plus what the conditioning of the pattern
    # costs any fp32 evaluation, twice fp32 torch's own distance to fp64 (P2's levels of -200 / -199 are mean / sigma = 400: half an ulp
    # of the fp32 mean is 1.5e-5 of the result there)
    pat = dc.pattern_of(cout)
    pat[cin:] = dc.PATTERNS
    g, o = nchw(got, b, ho, wo).double().cpu(), nchw(own, b, ho, wo).double().cpu()
    for p in range(dc.PATTERNS + (cout > cin)):
        sel = pat == p
        e = (g[:, sel] - o[:, sel]).abs().max().item()
        e32 = (n32[:, sel].double() - n64[:, sel]).abs().max().item()
        bound = 2 * e32 + 1e-5 * max(1.0, n64[:, sel].abs().max().item())
        record(what + ' epilogue vs own', f'P{p}', e, e32, bound)
        assert e <= bound, (what, p, e, bound)


def test_norm_on_load_convolution_on_the_patterns(ops, lib):
    """``ops.conv2d_nhwc_normed`` at the first supported geometry of tests/test_conv_norm_on_load_gpu.py: bit for bit
    ``nhwc_norm`` + ``conv2d_nhwc`` (that file's contract), and against fp64 of conv2(relu(instance_norm(y))) with ``y`` the first
    convolution's own output read back (test_on_load_convolution_matches_fp64: 4e-6 relative; the normalised operand is in z units, so
    the statistics' error enters through the pattern gates of the operand, checked on the normalisation pass above)."""
    from tests.test_conv_norm_on_load_gpu import CASES
    c, (h, w), b = next(g for g in CASES if lib.um_conv2d_norm_supported(g[1][0], g[1][1], g[0], g[0], 3, 3, 1, 1, 1, 0))
    x = dc.channel_patterns(b, 64, h, w, seed=4400)
    w1, b1 = dc.pattern_conv_weights(c, 64, 3, 4401)
    w2 = rnd(4403, c, c, 3, 3, scale=0.06)
    planes, _ = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=True)
    y, _, _ = ops.conv2d_nhwc((planes, b, h, w, 64), w1.to(DEV), b1.to(DEV), 1, (1, 1), stats=True)
    st = ops.last_conv_stats
    tp, tf = ops.nhwc_norm(y, b, h * w, relu=True, want_planes=True, want_f32=True, conv_stats=st)
    ua, _, _ = ops.conv2d_nhwc((tp, b, h, w, c), w2.to(DEV), None, 1, (1, 1), stats=True)
    sta = ops.last_conv_stats[0].clone()
    (ub, _, _), counts = census(lib, lambda: ops.conv2d_nhwc_normed(y, st, (b, h, w, c), w2.to(DEV), None, stats=True))
    assert counts['conv_patch_norm'] == 1, counts
    assert torch.isfinite(ub).all()
    assert torch.equal(ua, ub), err(ua, ub)
    assert torch.equal(sta, ops.last_conv_stats[0])
    # the operand the kernel normalised, against fp64 of the first convolution's own output
    n64, n32 = norm_of_own_output(y, b, h, w)
    ym = nchw(y, b, h, w).cpu()
    dc.check_output_patterns(ym, 64)                                   # the patterns reached the first convolution's output
    pattern_gates(f'norm on load {c} {(h, w)} operand', nchw(tf, b, h, w), n64.relu(), n32.relu(), 3e-5, carry=64)
    constant_channel_gate(f'norm on load {c} {(h, w)} operand', nchw(tf, b, h, w), ym, carry=64)
    # ... and the convolution of that operand: fp64 of the operand the kernel built (read back), the convolution's own tolerance
    want = F.conv2d(nchw(tf, b, h, w).double().cpu(), w2.double(), None, padding=1)
    e = err(nchw(ub, b, h, w), want)[0]
    bound = 4e-6 * max(1.0, want.abs().max().item())
    record(f'norm on load {c} {(h, w)} convolution', 'all', e, bound, bound)
    assert e < bound


def test_entry_convolution_on_the_patterns(ops, lib):
    """``ops.conv2d_entry`` with the shortcut's own norm at the first supported geometry of tests/test_conv_entry_gpu.py: bit for bit
    ``nhwc_norm(u, shortcut_planes=)`` -> two ``conv2d_nhwc`` (that file's contract); the block input X the parent sequence writes is
    gated per pattern against fp64 of ``u`` read back; the projection's raw output through ``nhwc_norm(shortcut_stats=)`` against fp64
    of the two outputs read back (test_entry_convolution_matches_fp64: 4e-6 relative for the convolutions)."""
    from tests.test_conv_entry_gpu import CASES
    cin, cout, (h, w), b = next(g for g in CASES if lib.um_conv2d_entry_supported(g[2][0], g[2][1], g[0], g[1], 3, 3, 2, 1, 1, 0))
    s = dc.channel_patterns(b, cin, h, w, seed=4500)
    w0, b0 = dc.pattern_conv_weights(cin, cin, 3, 4501)
    w1, (wpj, bpj) = rnd(4503, cout, cin, 3, 3, scale=0.06), dc.pattern_conv_weights(cout, cin, 1, 4504)
    sp, _ = ops.nchw_to_nhwc(s.to(DEV).contiguous(), want_planes=True)
    u, _, _ = ops.conv2d_nhwc((sp, b, h, w, cin), w0.to(DEV), b0.to(DEV), 1, (1, 1), stats=True)
    stu = ops.last_conv_stats
    xp, xf = ops.nhwc_norm(u, b, h * w, relu=True, shortcut_planes=sp, want_planes=True, want_f32=True, conv_stats=stu)
    ta, ho, wo = ops.conv2d_nhwc((xp, b, h, w, cin), w1.to(DEV), None, 2, (1, 1), stats=True)
    sta = ops.last_conv_stats[0].clone()
    da, _, _ = ops.conv2d_nhwc((xp, b, h, w, cin), wpj.to(DEV), bpj.to(DEV), 2, (0, 0), stats=True)
    sda = ops.last_conv_stats[0].clone()
    (tb, db, ho2, wo2, st_t, st_d), counts = census(lib, lambda: ops.conv2d_entry(u, stu, sp, (b, h, w, cin), w1.to(DEV), wpj.to(DEV), bpj.to(DEV)))
    assert (ho2, wo2) == (ho, wo) and counts['conv_generic'] == 1, counts
    for name, p, q in (('t', ta, tb), ('d', da, db), ('t statistics', sta, st_t[0]), ('d statistics', sda, st_d[0])):
        assert torch.isfinite(q).all(), name
        assert torch.equal(p, q), (name, err(p, q))
    # X = relu(instance_norm(u) + S) per pattern, fp64 of u read back; S as the planes hold it (hi + lo)
    n64, n32 = norm_of_own_output(u, b, h, w)
    dc.check_output_patterns(nchw(u, b, h, w).cpu(), cin)              # the patterns reached u
    spf = nchw(sp.view(torch.float16).view(2, b * h * w + 1, cin)[:, :-1].float().sum(0), b, h, w).cpu()
    pattern_gates(f'entry {cin}->{cout} {(h, w)} block input', nchw(xf, b, h, w), (n64.relu() + spf.double()).relu(), (n32.relu() + spf).relu(), 3e-5)
    _, un = ops.nhwc_norm(u, b, h * w, relu=False, want_planes=False, want_f32=True, conv_stats=stu)
    constant_channel_gate(f'entry {cin}->{cout} {(h, w)} norm of u', nchw(un, b, h, w), nchw(u, b, h, w).cpu())
    xr = nchw(xf, b, h, w).double().cpu()
    for name, got, want in (('t', tb, F.conv2d(xr, w1.double(), None, stride=2, padding=1)), ('d', db, F.conv2d(xr, wpj.double(), bpj.double(), stride=2))):
        e = err(nchw(got, b, ho, wo), want)[0]
        bound = 4e-6 * max(1.0, want.abs().max().item())
        record(f'entry {cin}->{cout} {(h, w)} {name}', 'all', e, bound, bound)
        assert e < bound, name
    # the shortcut's own norm on load: relu(instance_norm(t) + instance_norm(d)), both from the tile statistics of the entry launch
    _, got = ops.nhwc_norm(tb, b, ho * wo, relu=True, shortcut=db, want_planes=False, want_f32=True, conv_stats=st_t, shortcut_stats=st_d)
    t64, t32 = norm_of_own_output(tb, b, ho, wo)
    d64, d32 = norm_of_own_output(db, b, ho, wo)
    # d = the patterns of X = relu(instance_norm(u) + S) at stride 2 (the 1x1 projection is the identity plus pattern-preserving
    # cross-talk): constant where u and S are constant, P3 / P4 at mean / sigma above 50 / 200 (X adds a unit-sigma term to S; P1 and
    # P6 do not survive the normalisation in X); t is textured in every channel and is the ``also`` term
    dm = nchw(db, b, ho, wo).cpu()
    dc.check_output_patterns(dm, cin, p4_ratio=200.0, patterns=(0, 3, 4))
    what = f'entry {cin}->{cout} {(h, w)} shortcut normalised on load'
    pattern_gates(what, nchw(got, b, ho, wo), (t64.relu() + d64).relu(), (t32.relu() + d32).relu(), 3e-5, also=t64, carry=cin)
    # the constant channels of d: its normalisation adds 0 (within one rounding of the mean) to relu(instance_norm(t)), which the
    # plain route gives from the same tile statistics
    _, tn = ops.nhwc_norm(tb, b, ho * wo, relu=True, want_planes=False, want_f32=True, conv_stats=st_t)
    constant_channel_gate(what, nchw(got, b, ho, wo) - nchw(tn, b, ho, wo), dm, carry=cin, slack=2.0 ** -23 * tn.abs().max().item())


@pytest.mark.parametrize('kind', ['black', 'letterbox', 'sensor_noise'])
def test_stem_conv_on_degenerate_images(ops, kind):
    """``ops.stem_conv(normalize=True)`` (test_stem_conv_matches_fp64: 4e-6 relative) on a black, a letterboxed and a noise-only
    0..255 image, and its statistics epilogue through ``nhwc_norm(conv_stats=)`` against fp64 of its own output (3e-5, as the
    convolution epilogue's test; a black image gives channels that are constant away from the border)."""
    case = ff.BY_NAME['flow_s1_split1']                      # 0..255 images, (64, 96)
    img = torch.cat(dc.pair(case, kind), 0)
    b, _, h, w = img.shape
    wt = rnd(4600, 64, 3, 7, 7, scale=0.12)
    mean, std = dc.IMAGENET_MEAN, dc.IMAGENET_STD
    x = (img.double() / 255.0 - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    want = F.conv2d(x, wt.double(), None, stride=2, padding=3)
    got, ho, wo = ops.stem_conv(img.to(DEV).contiguous(), wt.to(DEV), (mean, std))
    st = ops.last_conv_stats
    assert (ho, wo) == tuple(want.shape[-2:])
    e = err(nchw(got, b, ho, wo), want)[0]
    bound = 4e-6 * max(1.0, want.abs().max().item())
    record(f'stem_conv {kind}', 'all', e, bound, bound)
    assert torch.isfinite(got).all() and e < bound
    _, y = ops.nhwc_norm(got, b, ho * wo, relu=True, want_planes=False, want_f32=True, conv_stats=st)
    _, own = ops.nhwc_norm(got, b, ho * wo, relu=True, want_planes=False, want_f32=True)
    n64, n32 = norm_of_own_output(got, b, ho, wo)
    e32 = (n32.double() - n64).abs().max().item()
    for name, t in (('epilogue statistics', y), ('own pass', own)):
        e = err(nchw(t, b, ho, wo), n64.relu())[0]
        bound = 2 * e32 + 3e-5 * max(1.0, n64.abs().max().item())
        record(f'stem_conv {kind} norm, {name}', 'all', e, e32, bound)
        assert torch.isfinite(t).all() and e <= bound, (kind, name, e, bound)


# ------------------------------------------------------------------ LayerNorm epilogues
def _layer_norm(seed):
    norm = torch.nn.LayerNorm(128)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(seed, 128))
        norm.bias.copy_(0.1 * rnd(seed + 1, 128))
    return norm


def row_gates(what, got, want64, want32, group, tol):
    """Zero, identical and control rows under the entry point's own tolerance, offset rows under 2 x fp32 torch + that tolerance."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    for gi, name in enumerate(dc.ROW_GROUPS):
        sel = group == gi
        assert bool(sel.any()), (what, name)
        e = (got[sel] - want64[sel]).abs().max().item()
        e32 = (want32[sel].double() - want64[sel]).abs().max().item()
        bound = 2 * e32 + tol if name == 'offset' else tol
        record(what, name + ' rows', e, e32, bound)
        assert e <= bound, (what, name, e, bound)


def test_linear_layernorm_on_degenerate_rows(ops):
    """``ops.linear_ln`` at the size of test_linear_layernorm_residual (2e-5): rows of exact zeros (the pre-norm vector is exactly
    constant: the result is ``beta`` plus the residual), a block of bitwise-identical rows, and rows whose pre-norm vector carries a
    common offset of 10^2 sigma (input column 0 is 8 on those rows and 0 elsewhere, weight column 0 is 28: sigma of the rest is 2.3)."""
    m = 333
    a, group = dc.token_rows(m, 128, seed=4700, scale=2.0)
    w = rnd(4701, 128, 128, scale=0.1)
    a[:, 0] = torch.where(group == 2, 8.0, 0.0)
    w[:, 0] = 28.0
    res = rnd(4702, m, 128)
    norm = _layer_norm(4703)
    ln = lambda t: F.layer_norm(t, (128,), norm.weight.to(t.dtype), norm.bias.to(t.dtype), norm.eps)
    pre64 = a.double() @ w.double().t()
    off = pre64[group == 2]
    assert 50 < (off.mean(1) / off.std(1)).min().item()
    want64, want32 = ln(pre64), ln(a @ w.t())
    zero = group == 0
    assert torch.equal(want64[zero], norm.bias.double().expand(int(zero.sum()), 128))
    normd = _layer_norm(4703).to(DEV)
    got = ops.linear_ln(a.to(DEV), (w.to(DEV),), normd)
    row_gates('linear_ln', got, want64, want32, group, 2e-5)
    record('linear_ln', 'zero rows exactly beta', bool(torch.equal(got.cpu()[zero], norm.bias.expand(int(zero.sum()), 128))))
    ident = torch.nonzero(group == 1).flatten()
    first_run = ident[:16]
    assert torch.equal(got[first_run].cpu(), got[first_run[:1]].cpu().expand(16, 128))        # identical rows: identical results
    got = ops.linear_ln(a.to(DEV), (w.to(DEV),), normd, residual=res.to(DEV))
    row_gates('linear_ln residual', got, want64 + res.double(), want32 + res, group, 2e-5)


def test_ffn_layernorm_on_degenerate_rows(ops):
    """``ops.ffn_ln`` at (333, 1024) of test_fused_ffn_kernel (3e-5).  Zero rows of x and y give gelu(0) = 0: the result is ``x + beta``.
    The offset enters through one hidden unit that reads x[:, 0] alone (6 on the offset rows, 0 elsewhere) and feeds every output
    with weight 38: about 10^2 sigma of the pre-norm vector."""
    m, hidden = 333, 1024
    x, group = dc.token_rows(m, 128, seed=4800, scale=1.5)
    y = rnd(4801, m, 128, scale=1.5)
    y[group == 0] = 0.0
    y[group == 1] = y[int(torch.nonzero(group == 1)[0])].clone()
    x[:, 0] = torch.where(group == 2, 6.0, 0.0)
    w1 = rnd(4802, hidden, 256, scale=0.08)
    w2 = rnd(4803, 128, hidden, scale=0.06)
    w1[:, 0] = 0.0
    w1[7] = 0.0
    w1[7, 0] = 1.0
    w2[:, 7] = 38.0
    norm = _layer_norm(4804)
    want64 = ffn_reference(x, y, w1, w2, norm)
    hid32 = F.gelu(torch.cat([x, y], 1) @ w1.t())
    want32 = x + F.layer_norm(hid32 @ w2.t(), (128,), norm.weight, norm.bias, norm.eps)
    pre = F.gelu(torch.cat([x, y], 1).double() @ w1.double().t()) @ w2.double().t()
    assert 50 < (pre[group == 2].mean(1) / pre[group == 2].std(1)).min().item()
    zero = group == 0
    assert torch.equal(want64[zero], norm.bias.double().expand(int(zero.sum()), 128))          # x is 0 there too
    got = ops.ffn_ln(x.to(DEV), y.to(DEV), w1.to(DEV), w2.to(DEV), _layer_norm(4804).to(DEV))
    row_gates('ffn_ln', got, want64, want32, group, 3e-5)
    record('ffn_ln', 'zero rows exactly beta', bool(torch.equal(got.cpu()[zero], norm.bias.expand(int(zero.sum()), 128))))
    # the bf16 throughput mode, as in test_fused_ffn_kernel (bf16-level agreement), on the rows whose conditioning allows it: the
    # offset rows carry 228 in every pre-norm element, where one bf16 rounding of the hidden unit (2^-9 relative) is a fifth of sigma
    fast = HipOps('fast').ffn_ln(x.to(DEV), y.to(DEV), w1.to(DEV), w2.to(DEV), _layer_norm(4804).to(DEV))
    assert torch.isfinite(fast).all()
    plain = group != 2
    e_fast = err(fast[plain.to(DEV)], want64[plain])
    record('ffn_ln fast mode', 'max, mean off the offset rows', e_fast[0], e_fast[1], 0.5)
    assert e_fast[1] < 2e-2 and e_fast[0] < 0.5, e_fast


@pytest.mark.parametrize('shifted,residual', [(False, True), (True, False)])
def test_attention_merge_layernorm_on_degenerate_streams(ops, shifted, residual):
    """``ops.window_attention_merge`` at the size of test_attention_merge_and_kv_rotate (5e-5), the degenerate content per stream (stream
    s reads the keys / values of stream s + 2): the values of stream 2 are zero, so every row of stream 0 is exactly ``beta`` (+
    residual); the tokens of streams 1 and 3 are one vector each, so stream 1 gives identical rows; the values of stream 0 carry one
    constant channel that the merge weight spreads over every output, a common offset of about 10^2 sigma for stream 2; stream 3 is
    the control."""
    s_, h, w, c = 4, 16, 24, 128
    l = h * w
    x = rnd(4900, s_ * l, c, scale=1.5).view(s_, l, c)
    xt = rnd(4901, s_ * l, c, scale=1.5).view(s_, l, c)
    x[1], xt[3] = x[1, :1].clone(), xt[3, :1].clone()
    xt[2] = 0.0
    xt[:, :, 0] = 0.0
    xt[0, :, 0] = 6.0
    x, xt = x.reshape(s_ * l, c).contiguous(), xt.reshape(s_ * l, c).contiguous()
    wq, wk, wv, wm = (rnd(4902 + i, c, c, scale=0.09) for i in range(4))
    wv[:, 0] = 0.0
    wv[5] = 0.0
    wv[5, 0] = 1.0                                   # value channel 5 = xt[:, 0]: 6 on stream 0, 0 elsewhere
    wm[:, 5] = 25.0
    group = torch.tensor([0, 1, 2, 3]).repeat_interleave(l)
    norm = _layer_norm(4906)
    geom = (8, 12, 4, 6) if shifted else (8, 12, 0, 0)
    rot = 2
    want64 = merged_layer_reference(x, xt, wq, wk, wv, wm, norm, s_, h, w, geom, rot, residual)
    # the same composition in fp32 torch
    q32 = (x @ wq.t()).view(s_, l, c)
    kv = xt.view(s_, l, c).roll(-rot, 0)
    att = hp.window_attention(q32, kv @ wk.t(), kv @ wv.t(), h, w, *geom)
    pre32 = att.reshape(s_ * l, c) @ wm.t()
    want32 = F.layer_norm(pre32, (c,), norm.weight, norm.bias, norm.eps) + (x if residual else 0.0)
    off = pre32[group == 2].double()
    assert 50 < (off.mean(1) / off.std(1)).min().item()
    zero = group == 0
    assert torch.equal(want64[zero] - (x.double()[zero] if residual else 0.0), norm.bias.double().expand(l, c))
    normd = _layer_norm(4906).to(DEV)
    xd, xtd = x.to(DEV), xt.to(DEV)
    qp, _, _ = ops.linear_planes(xd, (wq.to(DEV),))
    kvp, _, n2 = ops.linear_planes(xtd, (wk.to(DEV), wv.to(DEV)))
    m = s_ * l
    got = ops.window_attention_merge((qp, m, c, 0), (kvp, m, n2, 0), (kvp, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), normd, xd if residual else None)
    what = f'window_attention_merge shifted={int(shifted)} residual={int(residual)}'
    row_gates(what, got.reshape(m, c), want64, want32, group, 5e-5)
    got2 = ops.window_attention_qproj_merge(xd, wq.to(DEV), (kvp, m, n2, 0), (kvp, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), normd, xd if residual else None)
    row_gates(what + ' (q in the prologue)', got2.reshape(m, c), want64, want32, group, 5e-5)
    # bf16 operands, as in test_attention_merge_and_kv_rotate: the two forms agree with fp64 equally well
    fast = HipOps('fast')
    kvf, _, _ = fast.linear_planes(xtd, (wk.to(DEV), wv.to(DEV)))
    qpf, _, _ = fast.linear_planes(xd, (wq.to(DEV),))
    ref_f = fast.window_attention_merge((qpf, m, c, 0), (kvf, m, n2, 0), (kvf, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), normd, xd if residual else None)
    got_f = fast.window_attention_qproj_merge(xd, wq.to(DEV), (kvf, m, n2, 0), (kvf, m, n2, c), s_, h, w, *geom, rot, wm.to(DEV), normd, xd if residual else None)
    assert torch.isfinite(ref_f).all() and torch.isfinite(got_f).all()
    e_ref, e_got = err(ref_f.reshape(m, c), want64), err(got_f.reshape(m, c), want64)
    record(what + ' fast mode', 'mean planes, prologue', e_ref[1], e_got[1], 1.25 * e_ref[1] + 1e-4)
    assert e_got[1] < 1.25 * e_ref[1] + 1e-4 and e_got[0] < 2.5 * e_ref[0] + 1e-3, (e_ref, e_got)


# ================================================================== softmaxes and arg-maxes under exact ties
IDENTITY_PROJ = {f'feature_flow_attn.{n}_proj.{p}': (torch.eye(C, dtype=torch.float64) if p == 'weight' else torch.zeros(C, dtype=torch.float64))
                 for n in ('q', 'k') for p in ('weight', 'bias')}
GLOBAL_SHAPES = [(1, 7, 9), (36, 24, 40)]
_global_refs = {}


def global_reference(kind, shape):
    """Inputs and the fp64 answers of the global ops for one (kind, shape): computed once, shared, read-only."""
    key = (kind,) + tuple(shape)
    if key not in _global_refs:
        b, h, w = shape
        f0, f1 = dc.token_maps(kind, b, h, w)
        val = rnd(5000, b, 2, h, w, scale=3.0)
        d0, d1 = f0.double(), f1.double()
        _global_refs[key] = (f0, f1, val, hp.global_corr_softmax_flow(d0, d1, True), hp.global_corr_softmax_stereo(d0, d1),
                             hp.prop_global(d1, val.double(), IDENTITY_PROJ))
    return _global_refs[key]


@pytest.mark.parametrize('kind', dc.TOKEN_KINDS)
def test_global_matching_under_exact_ties(ops, lib, kind):
    """``global_corr_softmax_flow`` (one direction and both), ``global_corr_softmax_stereo`` and ``prop_global`` (queries = keys = the
    second map's tokens) against ``oracle.hotpath`` in fp64 with the gates of test_global_matching_random_shapes, at (1, 7, 9) -- one
    ragged key tile, gsv3 -- and (36, 24, 40) -- 15 key tiles, gsv4 (asserted through the census, as REACHES does)."""
    seen = {'gsv3': 0, 'gsv4': 0}
    for shape in GLOBAL_SHAPES:
        b, h, w = shape
        f0, f1, val, want, want_s, want_p = global_reference(kind, shape)
        t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
        got, counts = census(lib, lambda: ops.global_corr_softmax_flow(t0, t1, h, w, bidir=True))
        for k in seen:
            seen[k] += counts[k]
        assert torch.isfinite(got).all(), (kind, shape)
        mx, mean = err(got, want)
        record(f'global flow bidir {kind} {shape}', 'max, mean', mx, mean, 2e-3)
        assert mean < 1e-4 and mx < 2e-3, (kind, shape, mx, mean)
        one = ops.global_corr_softmax_flow(t0, t1, h, w)
        assert err(one, want[:b])[0] < 2e-3, (kind, shape)
        got_s = ops.global_corr_softmax_stereo(t0, t1, h, w)
        record(f'global stereo {kind} {shape}', 'max', err(got_s, want_s)[0], 1e-3, 1e-3)
        assert torch.isfinite(got_s).all() and err(got_s, want_s)[0] < 1e-3, (kind, shape)
        got_p = ops.prop_global(t1, t1, val.to(DEV), h, w)
        record(f'prop_global {kind} {shape}', 'max', err(got_p, want_p)[0], 2e-3, 2e-3)
        assert torch.isfinite(got_p).all() and err(got_p, want_p)[0] < 2e-3, (kind, shape)
    assert seen['gsv3'] > 0 and seen['gsv4'] > 0, seen


@pytest.mark.parametrize('hw,path', [((9, 11), 'k3_valu'), ((16, 24), 'k3_mfma')])
@pytest.mark.parametrize('kind', dc.TOKEN_KINDS)
def test_local_matching_under_exact_ties(ops, lib, kind, hw, path):
    """``local_corr_softmax`` at radius 4 on 9x11 (the VALU kernel) and 16x24 (the matrix cores; the census says which ran) and
    ``prop_local`` at radius 2 against ``oracle.hotpath`` in fp64: 2e-4, the tolerance of test_local_kernels_random_shapes and
    test_propagation_golden."""
    b, (h, w) = 2, hw
    f0, f1 = dc.token_maps(kind, b, h, w, seed=5100)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    want = hp.local_corr_softmax(f0.double(), f1.double(), 4)
    got, counts = census(lib, lambda: ops.local_corr_softmax(t0, t1, h, w, 4))
    assert counts[path] == 1 and counts['k3_valu'] + counts['k3_mfma'] == 1, counts
    e = err(got, want)[0]
    record(f'local_corr_softmax r4 {kind} {hw} {path}', 'max', e, 2e-4, 2e-4)
    assert torch.isfinite(got).all() and e < 2e-4, (kind, hw, e)
    want_s = hp.local_corr_softmax(f0.double(), f1.double(), 4, True)
    assert err(ops.local_corr_softmax(t0, t1, h, w, 4, one_d=True), want_s)[0] < 2e-4, (kind, hw)
    val = rnd(5101, b, 2, h, w, scale=3.0)
    want_p = hp.prop_local(f1.double(), val.double(), IDENTITY_PROJ, 2)
    got_p = ops.prop_local(t1, t1, val.to(DEV), h, w, 2)
    e = err(got_p, want_p)[0]
    record(f'prop_local r2 {kind} {hw}', 'max', e, 2e-4, 2e-4)
    assert torch.isfinite(got_p).all() and e < 2e-4, (kind, hw, e)


@pytest.mark.parametrize('geo', [(2, 12, 20, 12, 20, 0, 0), (4, 6, 10, 3, 5, 1, 2)], ids=['plain', 'shifted'])
@pytest.mark.parametrize('kind', dc.TOKEN_KINDS)
def test_window_attention_under_exact_ties(ops, kind, geo):
    """``window_attention`` in one plain and one shifted geometry of ``WINDOWS`` (tests/test_memory_contract_gpu.py): queries and keys
    from the token kinds, textured values, against ``oracle.hotpath`` in fp64 with the gate of test_window_attention_random_geometries
    (5e-5 relative)."""
    s_, h, w, wh, ww, sh, sw = geo
    f0, f1 = dc.token_maps(kind, s_, h, w, seed=5200)
    q, k, v = tok(f0), tok(f1), rnd(5201, s_, h * w, C, scale=1.5)
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
    got = ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw)
    mx, _ = err(got, want)
    bound = 5e-5 * max(1.0, want.abs().max().item())
    record(f'window_attention {kind} {geo}', 'max', mx, bound, bound)
    assert torch.isfinite(got).all() and mx < bound, (kind, geo, mx)


@pytest.mark.parametrize('shape', [(2, 9, 15), (2, 24, 40)])
def test_match_stats_pick_the_lower_index_of_a_tie(shape):
    """``confidence.global_match_stats`` and ``um_match_mutual`` on ``duplicated`` tokens: every key of the upper half is a bitwise copy
    of a key of the lower half, so the two logits of a pair are equal whatever the accumulation order.  Where the fp64 maximum belongs
    to such a pair and its gap to the next distinct logit exceeds the tolerance of tests/test_match_stats_gpu.py, ``best`` must be the
    LOWER index of the pair -- the documented rule (match_stats.hip, confidence.py: "lowest index on a tie").  The float planes pass
    that file's gates, and ``mutual`` follows from the two ``best`` maps by the host expression."""
    from tests.test_match_stats_gpu import FIELDS, floors, gate, logits64
    b, h, w = shape
    l = h * w
    m0, m1 = dc.token_maps('duplicated', b, h, w, seed=5300)
    f0, f1 = tok(m0), tok(m1)
    partner = dc.duplicate_partner(l)
    assert torch.equal(f1[:, partner], f1) and int((partner != torch.arange(l)).sum()) == l // 2
    ref64 = confidence.global_match_stats_host(f0.double(), f1.double(), h, w, bidir=True)
    ref32 = confidence.global_match_stats_host(f0, f1, h, w, bidir=True)
    got = confidence.global_match_stats(f0.to(DEV), f1.to(DEV), h, w, bidir=True)
    fl = floors(h, w, False)
    for name in FIELDS:
        gate(name, getattr(got, name), getattr(ref64, name), getattr(ref32, name), fl[name], f'duplicated {shape}')
    # the forward direction's logits on the distinct keys only, then spread over the pairs: exactly equal within a pair by construction
    uniq = l - l // 2
    lg = logits64(f0.double(), f1.double()[:, :uniq], h, w, False)
    lg32 = logits64(f0, f1[:, :uniq], h, w, False)
    tol = 2 * (lg32.double() - lg).abs().max().item() + lg.abs().max().item() * 2.0 ** -20
    top2 = lg.topk(2, -1)
    winner = top2.indices[..., 0]                                         # a lower index: the distinct keys are the lower ones
    paired = winner < l // 2                                               # ... which has a copy in the upper half
    clear = (top2.values[..., 0] - top2.values[..., 1]) > tol
    decided = paired & clear
    assert decided.float().mean().item() > 0.2, decided.float().mean().item()
    best = got.best.cpu().view(2 * b, l).long()
    fwd, bwd = best[:b], best[b:]
    wrong = decided & (fwd != winner)
    upper = decided & (fwd == winner + uniq)
    record(f'match stats tie {shape}', 'decided rows, upper index taken, other', int(decided.sum()), int(upper.sum()), int((wrong & ~upper).sum()))
    assert not bool(wrong.any()), (shape, int(wrong.sum()), int(upper.sum()))
    # every row: a key whose fp64 logit is the row maximum within the tolerance (the other file's rule)
    full = lg[..., partner]
    assert bool((full.gather(-1, fwd[..., None])[..., 0] >= top2.values[..., 0] - tol).all())
    want_mutual = confidence.mutual_matches_host(fwd.view(b, h, w), bwd.view(b, h, w), h, w, 0)
    got_mutual = confidence.mutual_matches(got.best[:b], got.best[b:], h, w, 0)
    assert torch.equal(got_mutual.cpu(), want_mutual) and 0 < int(want_mutual.sum()) < b * l


# ================================================================== whole forwards
def forward_answers(case, kind):
    return dc.oracle(case, kind, torch.float64), dc.oracle(case, kind, torch.float32)


@pytest.mark.parametrize('name,kind', dc.MATRIX, ids=[f'{n}-{k}' for n, k in dc.MATRIX])
def test_forward_on_degenerate_content(name, kind):
    """One exact-mode forward per (case, kind) against the fp64 oracle under the per-sample gates of tests/test_forward_flags_gpu.py
    (mean <= 3 mean(e32) + 1e-4, max <= 3 max(e32) + MAX_FLOOR, the arg-max depth cap), ``check_operand_range`` after the forward."""
    case = ff.BY_NAME[name]
    (pred,), _ = run_gpu(case, images=dc.pair(case, kind))
    check_gates(case, pred, forward_answers(case, kind), tag=' ' + kind)


def test_forward_on_degenerate_content_as_two_parts():
    """(flow_s2_rr2_b2, fade) as two half-batch forwards on two streams (``launch_parts = 2``): the same bits as the whole-batch
    forward, and the same gates."""
    name, kind = dc.TWO_PARTS
    case = ff.BY_NAME[name]
    images = dc.pair(case, kind)
    (whole,), _ = run_gpu(case, images=images)
    (first, second), _ = run_gpu(case, parts=2, calls=2, images=images)
    assert torch.equal(first, second), (first - second).abs().max().item()
    assert torch.equal(whole, second), (whole - second).abs().max().item()
    check_gates(case, second, forward_answers(case, kind), tag=' ' + kind + ' two parts')


def test_sequence_on_degenerate_frames():
    """``forward_sequence`` over [t0, t0, black, t1, t1 letterboxed] at 64x96 on gmflow_s1 against the pairwise forwards with the
    comparator of test_sequence_against_pairwise (``floor_close``: 1e-3 relative to the flow's range; the repeat of the call and the
    device-side consistency check stay bitwise, as there)."""
    from tests.test_video_gpu import floor_close
    from unimatch_amd import video
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, **CONDITIONED))
    model = model.to(DEV)
    kw = {k: v for k, v in fk.items() if k != 'task'}
    frames = dc.frames('mixed').to(DEV)
    n = frames.shape[0]
    h, w = dc.SEQUENCE_SIZE
    pairwise = torch.cat([model(frames[i:i + 1], frames[i + 1:i + 2], pred_bidir_flow=True, **kw)['flow_preds'][0] for i in range(n - 1)],
                         0).view(n - 1, 2, 2, h, w)
    args = dict(pairs_per_launch=2, pred_bidir_flow=True, consistency_check=True, **kw)
    out = model.forward_sequence(frames, **args)
    assert torch.isfinite(out['flow']).all() and torch.isfinite(out['flow_bwd']).all()
    for i in range(n - 1):
        record(f'sequence pair {i}', 'max fwd, bwd', (out['flow'][i] - pairwise[i, 0]).abs().max().item(),
               (out['flow_bwd'][i] - pairwise[i, 1]).abs().max().item(), 1e-3 * max(1.0, pairwise[i, 0].abs().max().item()))
        assert floor_close(out['flow'][i], pairwise[i, 0]), i
        assert floor_close(out['flow_bwd'][i], pairwise[i, 1]), i
    again = model.forward_sequence(frames, **args)
    torch.cuda.synchronize()
    for key in ('flow', 'flow_bwd', 'occ_fwd', 'occ_bwd'):
        assert torch.equal(again[key], out[key]), key
    occ_f, occ_b = video.forward_backward_consistency_check(out['flow'], out['flow_bwd'])
    assert torch.equal(occ_f, out['occ_fwd']) and torch.equal(occ_b, out['occ_bwd'])
    model.check_operand_range()
