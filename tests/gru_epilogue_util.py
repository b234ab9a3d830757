"""Shared helpers of tests/test_gru_epilogue_cpu.py and tests/test_gru_epilogue_gpu.py: the gated / addend epilogue of the convolutions
(um_conv2d_gru_fwd, um_conv2d_gru_add_fwd: conv.hip, conv_epilogue_pass, the GATE and ADD branches of store_rows) one launch at a time.

Here: the float64 reference of ONE launch of each gate, written from the arithmetic of unimatch_amd/refine.py::_SepConvGRU.forward
with an optional addend on the pre-activation; the table of cases (the smallest shapes at which each thing can still go wrong, with
the kernel family each one means to reach); the operand layout of a launch (the refinement block's own column offsets); seeded inputs
at scales that keep every gate away from saturation; and mutants of the reference, which the host file uses to show that these inputs
make the device test able to fail.  Nothing here needs a GPU."""
import functools

import torch

from tests.dispatch_boundaries import conv_kind, rnd

F = torch.nn.functional

GATE_REL = 3e-6                   # x max(1, max|pre|): the gate of um_conv2d_ex outputs (test_conv2d_ex_random_geometries).  It carries over:
                                  # sigmoid, tanh, r -> r h and q -> (1 - z) h + z q are 1-Lipschitz in the pre-activation for |h| <= 1, z in [0, 1]
PRE_LIMIT = 10.0                  # max|pre| of every case stays below (asserted): the gate is at most 3e-5
MUTANT_MARGIN = 5.0               # every mutant differs from the reference by at least this many gates


def value_gate(pre):
    return GATE_REL * max(1.0, pre.abs().max().item())


def record(tag, gate, form, family, worst, gate_value):
    """One line per launch: what profiles/gru_epilogue.txt holds."""
    print(f'GRU-EPILOGUE | {tag} | gate {gate} | {form} | {family} | worst {worst:.3e} | gate {gate_value:.3e}')


# ------------------------------------------------------------------ the case table
# (tag, b, h, w, C, cin, ksize): C = channels of the hidden state, cin = input channels of the PLAIN launch (the hoisted launches of a
# C = 128 row read 128 / 256 of them, see layout()).  Row-window kernel: 256-pixel tiles, 8 waves; generic kernel: 128-pixel tiles, 4 waves.
K15, K51 = (1, 5), (5, 1)
CASES_128 = [
    # P = 323 >= 256: row-window kernel, two tiles per image, the second with 67 pixels (waves with 32, 32, 3, 0 ... valid rows); the
    # window runs past the start and the end of an image
    ('2x17x19-1x5', 2, 17, 19, 128, 384, K15),
    # P = 270, row-window; rows of 3 pixels: every pixel has masked taps; gate 1 = 3 images x 2 tiles x 2 channel tiles = 12 workgroups
    # (gate 2: 6), no multiple of the 8 XCDs: the remainder branch of xcd_remap
    ('3x90x3-1x5', 3, 90, 3, 128, 384, K15),
    ('1x16x16-1x5', 1, 16, 16, 128, 384, K15),           # P = 256: one exact tile of the row-window kernel
    ('1x15x17-1x5', 1, 15, 17, 128, 384, K15),           # P = 255: the generic kernel, the other side of conv_pick's threshold
    ('2x9x11-1x5', 2, 9, 11, 128, 384, K15),             # generic, one ragged 99-pixel tile per image
    ('2x9x11-5x1', 2, 9, 11, 128, 384, K51),
    ('2x19x23-5x1', 2, 19, 23, 128, 384, K51),           # generic, four tiles per image, the last with 53 pixels
    ('3x3x90-5x1', 3, 3, 90, 128, 384, K51),             # columns shorter than the taps
]
# legal by the C ABI's argument checks (channels % 4 == 0, cin % 32 == 0), no product shape.  Gate 1: cout = 128 / 72 is ONE 128-wide
# tile with the z | r boundary in the middle of the tile and, at 72, dropped columns; gate 2: cout = 64 / 36 is NT = 2 and so the
# generic kernel even for 1x5
CASES_SMALL = [
    ('2x17x19-1x5-C64', 2, 17, 19, 64, 64, K15),
    ('2x17x19-1x5-C36', 2, 17, 19, 36, 64, K15),
    ('2x9x11-1x5-C64', 2, 9, 11, 64, 64, K15),
    ('2x9x11-1x5-C36', 2, 9, 11, 36, 64, K15),
]
CASES = CASES_128 + CASES_SMALL
BY_TAG = {c[0]: c for c in CASES}

# the family each row means to reach, stated by hand: {tag: (gate 1, gate 2)} as (kind, NT).  The host file holds conv_kind against it.
EXPECT = {
    '2x17x19-1x5': (('rows', 4), ('rows', 4)),
    '3x90x3-1x5': (('rows', 4), ('rows', 4)),
    '1x16x16-1x5': (('rows', 4), ('rows', 4)),
    '1x15x17-1x5': (('generic', 4), ('generic', 4)),
    '2x9x11-1x5': (('generic', 4), ('generic', 4)),
    '2x9x11-5x1': (('generic', 4), ('generic', 4)),
    '2x19x23-5x1': (('generic', 4), ('generic', 4)),
    '3x3x90-5x1': (('generic', 4), ('generic', 4)),
    '2x17x19-1x5-C64': (('rows', 4), ('generic', 2)),
    '2x17x19-1x5-C36': (('rows', 4), ('generic', 2)),
    '2x9x11-1x5-C64': (('generic', 4), ('generic', 2)),
    '2x9x11-1x5-C36': (('generic', 4), ('generic', 2)),
}

FORMS = {1: ('plain', 'addend'), 2: ('plain', 'addend', 'addend+hidden_out')}


def family(case, gate):
    """(kind, NT) conv_pick gives the launch of ``gate`` (cout = 2 C | C; the hoisted forms change cin only, which conv_pick ignores)."""
    _, _, h, w, c, _, (kh, kw) = case
    return conv_kind(h, w, 2 * c if gate == 1 else c, kh, kw, 1, kh // 2, kw // 2)


def layout(case, gate, form):
    """Operand layout of one launch -> dict(ld, a_coff, cin, p_coff): source columns [a_coff, a_coff + cin) and destination columns
    [p_coff, p_coff + C) of the SAME ``ld``-wide planes buffer.  C = 128: the block's own layouts (refine_nhwc.py) -- plain form
    G = h | inp | motion | r h: z | r reads 0..384 and writes r h at 384, q reads 128..512 and writes h at 0; hoisted form
    G = inp | h | motion | r h: z | r reads the 128 changing columns at 256 (pass 1), q the 256 at 256, r h goes to 384 and h to 128."""
    _, _, _, _, c, cin, _ = case
    if c == 128:
        if form == 'plain':
            return dict(ld=512, a_coff=0 if gate == 1 else 128, cin=cin, p_coff=384 if gate == 1 else 0)
        return dict(ld=512, a_coff=256, cin=128 if gate == 1 else 256, p_coff=384 if gate == 1 else 128)
    return dict(ld=256, a_coff=64, cin=cin, p_coff=136 if gate == 1 else 192)


# ------------------------------------------------------------------ float64 references of one launch
def conv_nhwc(x, weight, bias=None):
    """Same-size stride-1 convolution of ``x [b, h, w, cin]`` (float64) -> ``[b * h * w, cout]``."""
    kh, kw = weight.shape[-2:]
    y = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, padding=(kh // 2, kw // 2))
    return y.permute(0, 2, 3, 1).reshape(-1, weight.shape[0])


def fp16_hi(t):
    return t.to(torch.float16).to(t.dtype)


MUTANTS_1 = ('h_row_later', 'h_four_columns_later', 'addend_of_image_0', 'activation_before_addend', 'planes_hi_only')
MUTANTS_2 = MUTANTS_1 + ('z_swapped',)


def _pre(x, weight, bias, addend, mutant, act):
    """(pre-activation, activated) of one launch; the two addend mutants live here."""
    b, hh, ww, _ = x.shape
    conv = conv_nhwc(x, weight, bias)
    if addend is not None and mutant == 'addend_of_image_0':
        addend = addend[:hh * ww].repeat(b, 1)
    pre = conv if addend is None else conv + addend
    if addend is not None and mutant == 'activation_before_addend':
        return pre, act(conv) + addend
    return pre, act(pre)


def _h_of(h, mutant):
    if mutant == 'h_row_later':
        return h.roll(-1, 0)
    if mutant == 'h_four_columns_later':
        return h.roll(-4, 1)
    return h


def gate1(x, weight, bias, h, addend=None, mutant=None):
    """z | r launch: ``zr = sigmoid(conv(x) + b + addend)`` -> ``(pre [rows, 2C], z [rows, C], r * h [rows, C])``.  ``x [b, hh, ww, cin]``,
    ``h [rows, C]``, ``addend [rows, 2C] | None``: the fp32 tensors handed to the kernel, cast to double; weight ``[2C, cin, kh, kw]``."""
    c = h.shape[1]
    pre, zr = _pre(x, weight, bias, addend, mutant, torch.sigmoid)
    rh = zr[:, c:] * _h_of(h, mutant)
    return pre, zr[:, :c], (fp16_hi(rh) if mutant == 'planes_hi_only' else rh)


def gate2(x, weight, bias, h, z, addend=None, mutant=None, want_planes=False):
    """q launch: ``(pre [rows, C], (1 - z) h + z tanh(conv(x) + b + addend))``; with ``want_planes`` a third item, what the operand planes
    of the new state hold (the state itself, except under the planes mutant)."""
    pre, q = _pre(x, weight, bias, addend, mutant, torch.tanh)
    hm = _h_of(h, mutant)
    new = z * hm + (1 - z) * q if mutant == 'z_swapped' else (1 - z) * hm + z * q
    if want_planes:
        return pre, new, (fp16_hi(new) if mutant == 'planes_hi_only' else new)
    return pre, new


# ------------------------------------------------------------------ seeded inputs of one launch
def _seed(case, gate, form):
    return 7000 + 100 * CASES.index(case) + 10 * gate + FORMS[2].index(form)


def make_inputs(case, gate, form, draw=0):
    """fp32 inputs of one launch (CPU): ``buf [rows, ld]`` the whole planes buffer's content (source columns included, N(0, 1)), weight
    ``[cout, cin, kh, kw]`` ~ N(0, 2 / (5 cin)), bias and addend ~ N(0, 1) (plain form: no addend; the addend forms keep the bias, so
    that both additions of the epilogue are in every such launch), ``h = tanh(N(0, 1))``."""
    _, b, hh, ww, c, _, (kh, kw) = case
    lay = layout(case, gate, form)
    rows, cout, s = b * hh * ww, (2 * c if gate == 1 else c), _seed(case, gate, form) + 100000 * draw
    d = dict(lay=lay, rows=rows, cout=cout)
    d['buf'] = rnd(s, rows, lay['ld'])
    d['weight'] = rnd(s + 1, cout, lay['cin'], kh, kw, scale=(2.0 / (5 * lay['cin'])) ** 0.5)
    d['bias'] = rnd(s + 2, cout)
    d['addend'] = None if form == 'plain' else rnd(s + 3, rows, cout)
    d['h'] = torch.tanh(rnd(s + 4, rows, c))
    return d


@functools.lru_cache(maxsize=None)
def _draw(tag, gate, form):
    """The first draw of the launch's inputs whose pre-activation stays below PRE_LIMIT (|pre| has a standard deviation of about 2 over up
    to 2e5 values: one draw in ten has a value beyond 5 sigma).  Decided on the inputs and the float64 reference alone."""
    for draw in range(16):
        if _reference(tag, gate, form, None, draw)['pre'].abs().max().item() < PRE_LIMIT:
            return draw
    raise AssertionError(f'no draw of {tag} gate {gate} {form} keeps |pre| below {PRE_LIMIT}')


def reference(case, gate, form, mutant=None):
    """The inputs of one launch and its float64 reference.  Gate 2's ``z`` is gate 1's reference on inputs of its own (the same case, form
    'plain' or 'addend'), rounded to fp32: no launch takes an input from another launch's output.  -> dict of the inputs plus ``pre`` and
    gate 1: ``z``, ``rh``; gate 2: ``z32`` (fp32 input), ``new``, ``planes``.  Cached and shared: callers leave it unchanged."""
    return _reference(case[0], gate, form, mutant, _draw(case[0], gate, form))


@functools.lru_cache(maxsize=48)
def _reference(tag, gate, form, mutant, draw):
    case = BY_TAG[tag]
    _, b, hh, ww, c, _, _ = case
    d = make_inputs(case, gate, form, draw)
    lay = d['lay']
    x = d['buf'][:, lay['a_coff']:lay['a_coff'] + lay['cin']].double().view(b, hh, ww, lay['cin'])
    w64 = d['weight'].double()
    b64 = None if d['bias'] is None else d['bias'].double()
    a64 = None if d['addend'] is None else d['addend'].double()
    if gate == 1:
        d['pre'], d['z'], d['rh'] = gate1(x, w64, b64, d['h'].double(), a64, mutant)
        return d
    g1 = reference(case, 1, 'plain' if form == 'plain' else 'addend')
    d['z32'] = g1['z'].float()
    d['pre'], d['new'], d['planes'] = gate2(x, w64, b64, d['h'].double(), d['z32'].double(), a64, mutant, want_planes=True)
    return d


def outputs(d, gate):
    """The compared outputs of a reference() result."""
    return (d['z'], d['rh']) if gate == 1 else (d['new'], d['planes'])


def mutants_of(case, gate, form):
    """The mutants that are defined for this launch: the addend ones need an addend, and image 0's addend is every image's at batch 1."""
    out = []
    for m in (MUTANTS_1 if gate == 1 else MUTANTS_2):
        if m in ('addend_of_image_0', 'activation_before_addend') and form == 'plain':
            continue
        if m == 'addend_of_image_0' and case[1] == 1:
            continue
        out.append(m)
    return out


# ------------------------------------------------------------------ um_conv7_fwd at stride 1
CONV7_REL = 4e-6                  # x max(1, max|want|): the gate of test_stem_conv_matches_fp64
CONV7_SHAPES = [(1, 7, 7),        # the smallest the ABI admits
                (2, 9, 11),       # multi-image, small ragged tile
                (2, 17, 19),      # three 128-pixel tiles per image, the last ragged
                (1, 8, 130)]      # a padded row pitch (138) that is not the width rounded to 8
# (shape, image channels, cout): 128 outputs at every shape and channel count (8 = the ABI's maximum); NT = 2 and 3 at one shape each
CONV7_CASES = [(s, ch, 128) for s in CONV7_SHAPES for ch in (1, 2, 8)] + [((2, 9, 11), 2, 64), ((2, 17, 19), 2, 96)]


def conv7_inputs(shape, ch, cout, seed=0):
    b, h, w = shape
    s = 9000 + 10 * CONV7_SHAPES.index(shape) + ch + 1000 * seed
    return rnd(s, b, ch, h, w, scale=2.0), rnd(s + 100, cout, ch, 7, 7, scale=(2.0 / (49 * ch)) ** 0.5), rnd(s + 200, cout)


def conv7_reference(image, weight, bias):
    """relu(conv2d(.., padding=3) + bias) in float64 -> ``[b * h * w, cout]``."""
    y = F.conv2d(image.double(), weight.double(), bias.double(), padding=3).relu()
    return y.permute(0, 2, 3, 1).reshape(-1, weight.shape[0])
