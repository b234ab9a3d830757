"""Host side of tests/test_gru_epilogue_gpu.py: the float64 references of one gate launch (tests/gru_epilogue_util.py) ARE the
SepConvGRU's arithmetic, plain and hoisted; the case table reaches the kernel families it names; and the seeded inputs make the device
test able to fail -- every mutant of the reference lies at least five gates away from it.  No GPU."""
import pytest
import torch

from tests import gru_epilogue_util as gu
from unimatch_amd.refine import BasicUpdateBlock, _SepConvGRU
from unimatch_amd.refine_nhwc import NhwcUpdateBlock

PASSES = (('1', (1, 5)), ('2', (5, 1)))


def nhwc(t):
    """``[b, c, h, w]`` -> ``[b, h, w, c]``"""
    return t.permute(0, 2, 3, 1).contiguous()


def rows_of(t):
    return nhwc(t).reshape(-1, t.shape[1])


def chain_plain(gru, h, x, b, hh, ww):
    """The two passes of the GRU as gate1 / gate2 launches in the plain layout: z | r over (h | x), weights concatenated along the outputs as
    refine_nhwc.py does; q over (r h | x).  h ``[rows, 128]``, x ``[rows, 256]`` -> h"""
    for tag, _ in PASSES:
        z, r, q = (getattr(gru, f'conv{g}{tag}') for g in 'zrq')
        hx = torch.cat([h, x], 1).view(b, hh, ww, -1)
        _, zz, rh = gu.gate1(hx, torch.cat([z.weight, r.weight], 0), torch.cat([z.bias, r.bias], 0), h)
        _, h = gu.gate2(torch.cat([rh, x], 1).view(b, hh, ww, -1), q.weight, q.bias, h, zz)
    return h


def test_chained_references_reproduce_the_module():
    torch.manual_seed(11)
    b, hh, ww = 2, 6, 7
    gru = _SepConvGRU(128, 256).double()
    h, x = torch.tanh(torch.randn(b, 128, hh, ww, dtype=torch.float64)), torch.randn(b, 256, hh, ww, dtype=torch.float64)
    with torch.no_grad():
        want = gru(h, x)
        got = chain_plain(gru, rows_of(h), rows_of(x), b, hh, ww)
    assert (got - rows_of(want)).abs().max().item() < 1e-12


class _WeightsOnly:
    """What NhwcUpdateBlock._weights needs of HipOps: no cache, and the 'planes' of a weight are the weight."""

    def _cache_get(self, tag, tensors):
        return tag, None

    def _cache_put(self, key, tensors, value):
        return value

    def conv_weight_planes_from(self, weight):
        return weight


def test_hoisted_split_reproduces_the_unsplit_gates():
    """The invariant columns (context, and in pass 1 the initial state) go through a convolution into the addend, bias included; the changing
    columns go through the gate: NhwcUpdateBlock's own weight permutations (zr1i / zr1v, q1i / q1v, zr2i / zr2v, q2i / q2v) over its hoisted
    column order G = inp | h | motion | r h, launch by launch as iterate() issues them.  The parameters are fp32 values held in double
    (_weights keeps the biases as fp32)."""
    torch.manual_seed(12)
    b, hh, ww = 2, 5, 6
    block = BasicUpdateBlock().double()                           # initialised in fp32, so every parameter is an fp32 value
    wts = NhwcUpdateBlock(_WeightsOnly(), block, torch.nn.Conv2d(128, 256, 1).double())._weights()
    net0 = torch.tanh(torch.randn(b * hh * ww, 128, dtype=torch.float64))
    inp, motion = torch.randn(b * hh * ww, 128, dtype=torch.float64).relu(), torch.randn(b * hh * ww, 128, dtype=torch.float64)
    v = lambda *cols: torch.cat(cols, 1).view(b, hh, ww, -1)
    wb = lambda tag: (wts[tag][0].double(), None if wts[tag][1] is None else wts[tag][1].double())
    with torch.no_grad():
        want = chain_plain(block.gru, net0, torch.cat([inp, motion], 1), b, hh, ww)
        # begin(): the four tables
        p = {'zr1': gu.conv_nhwc(v(inp, net0), *wb('zr1i')), 'q1': gu.conv_nhwc(v(inp), *wb('q1i')),
             'zr2': gu.conv_nhwc(v(inp), *wb('zr2i')), 'q2': gu.conv_nhwc(v(inp), *wb('q2i'))}
        # iterate(): pass 1 reads motion (G 256..384) and net0 itself, pass 2 h | motion (G 128..384); q reads motion | r h (G 256..512)
        assert wb('zr1v')[1] is None and wb('q1v')[1] is None and wb('zr2v')[1] is None and wb('q2v')[1] is None
        _, z, rh = gu.gate1(v(motion), wb('zr1v')[0], None, net0, p['zr1'])
        _, h = gu.gate2(v(motion, rh), wb('q1v')[0], None, net0, z, p['q1'])
        _, z, rh = gu.gate1(v(h, motion), wb('zr2v')[0], None, h, p['zr2'])
        _, h = gu.gate2(v(motion, rh), wb('q2v')[0], None, h, z, p['q2'])
    assert (h - want).abs().max().item() < 1e-12
    # and the unhoisted weights of the block are the module's own: z | r as they are, q with r h moved behind x
    with torch.no_grad():
        hx = v(net0, inp, motion)
        _, z, rh = gu.gate1(hx, *wb('zr1'), net0)
        _, h1 = gu.gate2(v(inp, motion, rh), *wb('q1'), net0, z)
        zc, rc, qc = block.gru.convz1, block.gru.convr1, block.gru.convq1
        _, z0, rh0 = gu.gate1(hx, torch.cat([zc.weight, rc.weight], 0), torch.cat([zc.bias, rc.bias], 0), net0)
        _, h0 = gu.gate2(v(rh0, inp, motion), qc.weight, qc.bias, net0, z0)
    assert (h1 - h0).abs().max().item() < 1e-12


LAUNCHES = [(c, g, f) for c in gu.CASES for g in (1, 2) for f in gu.FORMS[g]]


@pytest.mark.parametrize('case', gu.CASES, ids=[c[0] for c in gu.CASES])
def test_inputs_keep_the_gates_open_and_mutants_are_far(case):
    """Per launch of the row: max|pre| < 10 (so the device gate is at most 3e-5), z spread over (0, 1), and every mutant of the reference
    -- h one row later, h four columns later, image 0's addend for every image, the activation before the addend, z and 1 - z swapped, planes
    with the fp16 high part only -- at least five device gates away in one of the compared outputs.  (The addend mutants need an addend;
    at batch 1 image 0's addend is the reference itself and is left out: gu.mutants_of.)"""
    for gate in (1, 2):
        for form in gu.FORMS[gate]:
            ref = gu.reference(case, gate, form)
            pre_max = ref['pre'].abs().max().item()
            assert pre_max < gu.PRE_LIMIT, (case[0], gate, form, pre_max)
            tol = gu.value_gate(ref['pre'])
            assert tol <= 3e-5
            z = ref['z'] if gate == 1 else ref['z32'].double()
            lo, hi = torch.quantile(z.flatten()[:100000], torch.tensor([0.05, 0.95], dtype=torch.float64)).tolist()
            assert lo < 0.15 and hi > 0.85, (case[0], gate, form, lo, hi)
            assert ref['h'].abs().max().item() <= 1.0
            muts = gu.mutants_of(case, gate, form)
            assert 'planes_hi_only' in muts and ('z_swapped' in muts) == (gate == 2)
            assert ('activation_before_addend' in muts) == (form != 'plain')
            for m in muts:
                mut = gu.reference(case, gate, form, m)
                far = max((a - b).abs().max().item() for a, b in zip(gu.outputs(mut, gate), gu.outputs(ref, gate)))
                print(f'MUTANT | {case[0]} | gate {gate} | {form} | {m} | {far:.3e} | gate {tol:.3e}')
                assert far >= gu.MUTANT_MARGIN * tol, (case[0], gate, form, m, far, tol)


def test_table_reaches_the_families_it_names():
    for case in gu.CASES:
        assert (gu.family(case, 1), gu.family(case, 2)) == gu.EXPECT[case[0]], case[0]
    for cases in (gu.CASES_128, gu.CASES):
        for gate in (1, 2):
            assert {gu.family(c, gate)[0] for c in cases} == {'rows', 'generic'}, gate
    # the two sides of conv_pick's 256-pixel threshold
    for gate in (1, 2):
        assert gu.family(gu.BY_TAG['1x16x16-1x5'], gate)[0] == 'rows' and gu.family(gu.BY_TAG['1x15x17-1x5'], gate)[0] == 'generic'
    # every C = 128 row is the block's own operand layout; every launch writes outside the columns it reads
    for case, gate, form in LAUNCHES:
        lay = gu.layout(case, gate, form)
        c = case[4]
        assert lay['a_coff'] + lay['cin'] <= lay['ld'] and lay['p_coff'] + c <= lay['ld']
        assert lay['p_coff'] >= lay['a_coff'] + lay['cin'] or lay['p_coff'] + c <= lay['a_coff']
        assert lay['cin'] % 32 == 0 and c % 4 == 0 and lay['a_coff'] % 8 == 0 and lay['p_coff'] % 4 == 0      # the C ABI's argument checks
    # what the issue's rows are about, as arithmetic on the table
    _, b, h, w, c, _, _ = gu.BY_TAG['3x90x3-1x5']
    tiles = b * ((h * w + 255) // 256)
    assert (tiles * 2) % 8 != 0 and tiles % 8 != 0                 # gate 1 (two channel tiles) and gate 2: the remainder branch of xcd_remap
    assert [min(32, max(0, 17 * 19 - 256 - 32 * wv)) for wv in range(4)] == [32, 32, 3, 0]


def test_conv7_cases():
    shapes = {s for s, _, _ in gu.CONV7_CASES}
    assert shapes == set(gu.CONV7_SHAPES)
    assert {(ch, co) for _, ch, co in gu.CONV7_CASES} >= {(1, 128), (2, 128), (8, 128), (2, 64), (2, 96)}
    assert (130 + 8 + 1) & ~1 != (130 + 7) // 8 * 8               # conv7_wp(130) = 138 (conv.hip): not the width rounded to 8
