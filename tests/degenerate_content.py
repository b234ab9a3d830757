"""Degenerate content: flat, black, letterboxed, noise-only and repeated frames, as plain data plus the helpers that build them.  No
pytest in here (the pattern of ``tests/forward_flags.py``): ``tests/test_degenerate_content_cpu.py`` and
``tests/test_degenerate_content_gpu.py`` read this one module.

Everything else in the suite feeds the kernels textured noise.  Video content is not like that: fades to black, letterbox bars, static
shots and duplicated frames drive the statistics kernels to zero variance and the softmaxes to exact ties.  Three families:

* ``pair(case, kind)`` / ``frames(kind)``: image pairs and a frame sequence for whole forwards (``KINDS``, ``MATRIX``);
* ``channel_patterns(b, c, h, w, seed)``: one NCHW tensor whose channels cycle through the eight statistics patterns ``P0 .. P7``;
* ``token_maps(kind, b, h, w)`` / ``token_rows(m, seed)``: feature maps that tie softmax logits exactly, and LayerNorm inputs with
  zero, identical and offset rows.
"""
import functools

import torch

from tests import forward_flags as ff
from unimatch_amd.synth import synth_frames

KINDS = ('black', 'white', 'grey_vs_black', 'identical', 'fade', 'letterbox', 'half_flat', 'sensor_noise')
_ALL_KINDS = ('flow_s1_split1', 'flow_s1_local', 'stereo_s1_local', 'stereo_s1_swin', 'depth_s1_localprop', 'depth_s1_argmax')
_FOUR_KINDS = ('flow_s2_rr2_b2', 'stereo_s2')
# (case name, kind): every row of the forward matrix
MATRIX = ([(c, k) for c in _ALL_KINDS for k in KINDS] + [(c, k) for c in _FOUR_KINDS for k in ('black', 'fade', 'letterbox', 'sensor_noise')]
          + [('flow_s2_rr3_bidir', 'identical')])
TWO_PARTS = ('flow_s2_rr2_b2', 'fade')                 # also run as two concurrent half-batch forwards: the same bits
E32_LIMIT = 1e-3                                        # the fp32 oracle stays this close to fp64: the GPU gates then mean something
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def pixel(case, v):
    """The pixel value ``v`` (0..255) in the case's input unit as ``[1, 3, 1, 1]``: 0..255 for flow, ImageNet-normalised otherwise."""
    if ff.task_of(case) == 'flow':
        return torch.full((1, 3, 1, 1), float(v))
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    return (float(v) / 255.0 - mean) / std


def _flat(like, value):
    return (torch.zeros_like(like) + value).contiguous()


def letterboxed(img, value):
    """``img`` with its top and bottom quarter at ``value``."""
    h = img.shape[-2]
    out = img.clone()
    out[..., :h // 4, :] = value
    out[..., h - h // 4:, :] = value
    return out.contiguous()


def pair(case, kind):
    """``(img0, img1)`` fp32 CPU tensors of the case's size and unit; the texture is the one of ``forward_flags.inputs(case)``."""
    t0, t1, _ = ff.inputs(case)
    black, grey, white = pixel(case, 0), pixel(case, 128), pixel(case, 255)
    if kind == 'black':
        return _flat(t0, black), _flat(t1, black)
    if kind == 'white':
        return _flat(t0, white), _flat(t1, white)
    if kind == 'grey_vs_black':
        return _flat(t0, grey), _flat(t1, black)
    if kind == 'identical':
        return t0.clone(), t0.clone()
    if kind == 'fade':
        return t0.clone(), _flat(t1, black)
    if kind == 'letterbox':
        return letterboxed(t0, black), letterboxed(t1, black)
    if kind == 'half_flat':
        out = []
        for t in (t0, t1):
            t = t.clone()
            t[..., :t.shape[-1] // 2] = grey
            out.append(t.contiguous())
        return tuple(out)
    if kind == 'sensor_noise':
        g = torch.Generator().manual_seed(case.seed + 77)
        out = []
        for t in (t0, t1):
            v = torch.randint(0, 3, tuple(t.shape), generator=g).float()
            if ff.task_of(case) != 'flow':
                v = (v / 255.0 - torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
            out.append(v.contiguous())
        return tuple(out)
    raise ValueError(f'unknown kind {kind!r}')


@functools.lru_cache(maxsize=None)
def _oracle(name, kind, dtype):
    case = ff.BY_NAME[name]
    i0, i1 = pair(case, kind)
    return ff.run_oracle(case, i0, i1, ff.inputs(case)[2], dtype)


def oracle(case, kind, dtype=torch.float64):
    """``oracle.model.unimatch_forward`` of ``pair(case, kind)`` in ``dtype``, computed once per process and shared: do not modify."""
    return _oracle(case.name, kind, dtype)


SEQUENCE_SIZE = (64, 96)


def frames(kind='mixed'):
    """``[5, 3, 64, 96]`` (0..255) for the sequence test: ``[t0, t0, black, t1, t1 letterboxed]`` -- a repeated frame, a cut to black and
    back, and letterbox bars appearing on a static shot."""
    if kind != 'mixed':
        raise ValueError(f'unknown kind {kind!r}')
    t = synth_frames(2, *SEQUENCE_SIZE, seed=2300)
    return torch.stack([t[0], t[0].clone(), torch.zeros_like(t[0]), t[1], letterboxed(t[1], 0.0)], 0).contiguous()


# ------------------------------------------------------------------ statistics patterns
PATTERNS = 8
P0_VALUES = (2.5, 0.0, -1000.0)
P2_LEVELS = ((1.0, -3.0), (0.0, 7.5), (-200.0, -199.0))


def pattern_of(c):
    """The pattern index of every channel ``[c]`` (channels cycle through P0 .. P7)."""
    return torch.arange(c) % PATTERNS


def p0_constant(c):
    """The constant of every channel ``[c]`` (meaningful on the P0 channels only)."""
    return torch.tensor(P0_VALUES)[(torch.arange(c) // PATTERNS) % len(P0_VALUES)]


def channel_patterns(b, c, h, w, seed):
    """One fp32 NCHW tensor whose channel ``ch`` holds pattern ``ch % 8``; the variant of a pattern (the constant of P0, the place of
    P1's pixel, the levels of P2) cycles with ``ch // 8``.  Every (sample, channel) plane draws from its own stretch of one seeded
    stream, so no two planes are equal and a sample swap cannot hide.

      P0  exactly constant (2.5, 0.0, -1000.0)
      P1  constant 2.5 except one pixel of 2.75 at flat index 0, the last index, or the middle
      P2  rows [0, h/4) and [3h/4, h) = a, the rest = b (a statistics chunk may be constant while chunks differ)
      P3  200 + N(0, 2^2): mean / sigma = 10^2
      P4  200 + N(0, 0.2^2): mean / sigma = 10^3
      P5  N(0, 1) with pixel (0, 0) = 1000 (the shift pixel is the outlier)
      P6  N(0, 1e-4^2): variance far below eps
      P7  N(0, 1): control
    """
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(b, c, h, w, generator=g)
    x = torch.empty(b, c, h, w)
    n = h * w
    for ch in range(c):
        p, variant = ch % PATTERNS, ch // PATTERNS
        z = noise[:, ch]
        if p == 0:
            x[:, ch] = P0_VALUES[variant % 3]
        elif p == 1:
            x[:, ch] = 2.5
            x[:, ch].view(b, n)[:, (0, n - 1, n // 2)[variant % 3]] = 2.75
        elif p == 2:
            lo, hi = P2_LEVELS[variant % 3]
            x[:, ch] = hi
            x[:, ch, :h // 4] = lo
            x[:, ch, (3 * h) // 4:] = lo
        elif p == 3:
            x[:, ch] = 200.0 + 2.0 * z
        elif p == 4:
            x[:, ch] = 200.0 + 0.2 * z
        elif p == 5:
            x[:, ch] = z
            x[:, ch, 0, 0] = 1000.0
        elif p == 6:
            x[:, ch] = 1e-4 * z
        else:
            x[:, ch] = z
    return x.contiguous()


# ------------------------------------------------------------------ softmax ties
TOKEN_KINDS = ('identical', 'zero', 'two_level', 'duplicated')
C = 128


def _randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def token_maps(kind, b, h, w, seed=3100):
    """``(f0, f1)`` fp32 feature maps ``[b, 128, h, w]`` (tokens: ``flatten(2).transpose(1, 2)``).

      identical   every token of both maps the same seeded vector (per sample)
      zero        all zeros
      two_level   the left half of both maps one vector, the right half another
      duplicated  textured ``f1`` whose second half of the token rows is a bitwise copy of the first half, with textured ``f0``
    """
    if kind == 'zero':
        return torch.zeros(b, C, h, w), torch.zeros(b, C, h, w)
    if kind == 'identical':
        f = _randn(seed, b, C, 1, 1).expand(b, C, h, w).contiguous()
        return f, f.clone()
    if kind == 'two_level':
        v = _randn(seed + 1, b, C, 2)
        f = torch.empty(b, C, h, w)
        f[..., :w // 2] = v[:, :, 0, None, None]
        f[..., w // 2:] = v[:, :, 1, None, None]
        return f, f.clone()
    if kind == 'duplicated':
        f0, f1 = _randn(seed + 2, b, C, h, w), _randn(seed + 3, b, C, h, w)
        f1 = 0.6 * f0.roll((1, -2), (2, 3)) + 0.4 * f1
        l = h * w
        t1 = f1.flatten(2).clone()
        t1[:, :, l - l // 2:] = t1[:, :, :l // 2]
        return f0.contiguous(), t1.view(b, C, h, w).contiguous()
    raise ValueError(f'unknown kind {kind!r}')


def duplicate_partner(l):
    """``[l]`` long: the lower token index that holds the same ``f1`` row in ``token_maps('duplicated')`` (itself where there is none)."""
    idx = torch.arange(l)
    upper = idx >= l - l // 2
    return torch.where(upper, idx - (l - l // 2), idx)


def uniform_centroid(h, w, dtype=torch.float64):
    """The expected coordinate ``[2]`` = (x, y) of a uniform softmax over all ``h * w`` keys."""
    return torch.tensor([(w - 1) / 2.0, (h - 1) / 2.0], dtype=dtype)


# ------------------------------------------------------------------ LayerNorm rows
ROW_GROUPS = ('zero', 'identical', 'offset', 'control')


def token_rows(m, k, seed, scale=1.0):
    """fp32 ``[m, k]`` for a LayerNorm epilogue, and the group of every row ``[m]`` as an index into ``ROW_GROUPS``: rows of exact
    zeros, blocks of bitwise-identical rows, the rows that are to carry a common offset of 10^2 sigma in the PRE-NORM vector (textured
    here: the offset has to pass the GEMM in front of the norm, so each test plants it through one input column and one weight
    column), and textured control rows, in runs of 16 .. 20 so that a 32-row tile holds more than one group."""
    x = _randn(seed, m, k, scale=scale)
    group = torch.full((m,), 3, dtype=torch.long)
    run, pos, which = 16, 0, 0
    while pos < m:
        group[pos:pos + run] = which % 4
        pos += run
        run = 16 + (run - 15) % 5
        which += 1
    x[group == 0] = 0.0
    x[group == 1] = x[int(torch.nonzero(group == 1)[0])].clone()
    return x.contiguous(), group


# ------------------------------------------------------------------ patterns through a convolution
def pattern_conv_weights(cout, cin, k, seed):
    """``(weight [cout, cin, k, k], bias [cout])`` that carry ``channel_patterns`` from a convolution's input into its OUTPUT: 1 at the
    centre tap on the diagonal plus ``0.01 * randn`` cross-talk, placed so that no pattern is destroyed --

      * from a P7 source (zero-mean unit noise) through all ``k * k`` taps into the P2, P3, P4, P5 and P7 outputs and into the outputs
        beyond ``cin`` (which carry no pattern: zero-mean mixtures);
      * from a P0 source (a constant: 2.5, 0 or -1000) through the centre tap alone into every patterned output but P6: a constant in
        gives the same constant out at every pixel, the zero-padded border included, so P0 stays exactly constant and P1 keeps its
        one pixel; the means move by up to about 20;
      * P6 (zero mean, variance far below eps) takes neither cross-talk nor bias: a mean of 10 there is mean / sqrt(var + eps) =
        3000, beyond the patterns' range -- half an ulp of the fp32 mean alone is then 1.5e-4 of the result.

    Cross-talk from every channel through every tap (the first version of these tests) turned the -1000 constants and the 1000 outlier
    into border steps of +-10 in all channels: no output was constant and mean / sigma fell to 10 .. 30."""
    g = torch.Generator().manual_seed(seed)
    noise = 0.01 * torch.randn(cout, cin, k, k, generator=g)
    wt = torch.zeros(cout, cin, k, k)
    src = pattern_of(cin)
    for o in range(cout):
        po = o % PATTERNS if o < cin else None
        if po is None or po in (2, 3, 4, 5, 7):
            wt[o, src == 7] = noise[o, src == 7]
        if po is not None:
            if po != 6:
                wt[o, src == 0, k // 2, k // 2] = noise[o, src == 0, k // 2, k // 2]
            wt[o, o, k // 2, k // 2] += 1.0
    bias = 0.5 * torch.randn(cout, generator=g)
    bias[:cin][src == 6] = 0.0
    return wt, bias


def check_output_patterns(y, carry, p4_ratio=500.0, patterns=(0, 1, 3, 4, 6)):
    """Asserts that ``y`` (NCHW, any float dtype), a convolution's output, still holds the patterns in its first ``carry`` channels: P0
    planes exactly constant, P1 planes constant but for one pixel, P6 zero-mean with a variance below 1e-2 eps, P3 / P4 with mean / sigma above 50 / ``p4_ratio`` (``patterns``: which of these to check)."""
    y = y.double()[:, :carry]
    pat = pattern_of(carry)
    flat = y.flatten(2)
    spread = flat.amax(-1) - flat.amin(-1)
    assert 0 not in patterns or bool((spread[:, pat == 0] == 0).all()), ('P0 is not constant', spread[:, pat == 0].max().item())
    for plane in flat[:, pat == 1].reshape(-1, flat.shape[-1]) if 1 in patterns else ():
        values, counts = plane.unique(return_counts=True)
        # (a stride-2 convolution steps over the pixel when it sits at an odd place: that plane is then constant)
        assert values.numel() <= 2 and (values.numel() == 1 or int(counts.min()) == 1), ('P1 is not one pixel on a constant', values.numel())
    assert 6 not in patterns or flat[:, pat == 6].var(-1, unbiased=False).max().item() < 1e-2 * 1e-5, 'P6 variance is not far below eps'
    assert 6 not in patterns or flat[:, pat == 6].mean(-1).abs().max().item() < 1e-4, 'P6 is not zero-mean'
    ratio = (flat.mean(-1) / flat.std(-1)).abs()
    assert 3 not in patterns or ratio[:, pat == 3].min().item() > 50, ('P3 mean / sigma', ratio[:, pat == 3].min().item())
    assert 4 not in patterns or ratio[:, pat == 4].min().item() > p4_ratio, ('P4 mean / sigma', ratio[:, pat == 4].min().item())
